"""The derived march kernels on the GPU across the scenario table of tests/_scenarios.py: every form built on
march_slot -- supersampled, adaptive, shutter, lens, ray map, ray-map lens, posed ray map, origin map -- at the
scene-flag folds, caps and uniform gates that the plain march is already held to, against the references of
tests/_ss_ref.py, _adaptive_ref.py, _shutter_ref.py, _lens_ref.py, _lens_mip_ref.py, _rays_ref.py, _rays_pose_ref.py and
_rays_origins_ref.py at that scenario: the CPU oracle's rays, resolved and encoded in numpy -- bit for bit.  The
reference is never the GPU's own output, except in the fast-math tests, which say why.  What each scenario aims at is
asserted from the oracle alone in tests/test_scenarios_host.py.

Every scenario renders in a fresh Scene of its cap and flags, four times: in the order of a fresh state, in the order
learned from that call's tile costs, and on each build of the exact kernels."""
import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests import _adaptive_ref, _lens_ref, _rays_origins_ref, _rays_pose_ref, _rays_ref, _shutter_ref
from tests import _scenarios as S
from tests._cases import camera_uniform
from tests._gpu_common import FAST_TOL, gpu_render
from tests._lens_mip_ref import shade_mip_np
from tests._ss_ref import expected_bytes, reference, resolve_np, scenario_uniforms, sky_ss

pytestmark = pytest.mark.gpu

F32, F16, BGRA8 = bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB
SENTINEL = 0xA5  # every byte of a buffer before a render (an fp32 / fp16 of all-0xA5 bytes is no value a frame holds)
GUARD = 4096     # bytes on either side of a target that no render may touch
T = bh.BH_SCHED_TILE
PASSES = [("fresh order", 0), ("learned order", 0), ("issue-order build", T | bh.BH_SCHED_FLAG_ISSUE_ORDER),
          ("latency build", T | bh.BH_SCHED_FLAG_LATENCY)]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Scene:
    """A fresh bh.Scene of the scenario's cap, flags and uniforms; closed on exit."""

    def __init__(self, s, math=bh.BH_MATH_EXACT):
        self.s, self.math = s, math

    def __enter__(self):
        self.sc = bh.Scene(16, 16, sky=sky_ss(), max_iters=self.s.cap, scene_flags=self.s.flags, math=self.math)
        self.sc.uniforms = scenario_uniforms(self.s.key)
        return self.sc

    def __exit__(self, *exc):
        self.sc.close()


class Target:
    """n bytes inside a sentinel-filled buffer with a guard region on either side (tests/test_gpu_shutter.py's);
    handed to the library as a raw device pointer."""

    def __init__(self, torch, shape, bytes_per):
        self.shape = tuple(shape) + (bytes_per,)
        self.n = int(np.prod(shape)) * bytes_per
        self.buf = torch.full((2 * GUARD + self.n,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD

    def bytes(self):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all(), "a store outside the target"
        return b[GUARD:GUARD + self.n].reshape(self.shape)


def pixels(torch, W, H, fmt=F32):
    return Target(torch, (H, W), _abi.BYTES_PER_PIXEL[fmt])


def assert_frame(got, want, what):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(got.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}"


def assert_pair(col, bo, ref, fmt, what):
    assert_frame(col.bytes(), expected_bytes(fmt, ref[0]), f"{what}: col")
    assert_frame(bo.bytes(), expected_bytes(fmt, ref[1]), f"{what}: blackout_col")


def upload(torch, m):
    return torch.from_numpy(np.array(m, dtype=np.float32, order="C")).cuda()  # a copy: the references are read-only


# ---- the forms, one call each -------------------------------------------------------------------------------------
def check_ss(torch, sc, s, W, H, k, fmt=F32, passes=PASSES):
    ref = reference(s.camera, W, H, k, s.key)
    sc.camera_uniform = camera_uniform(s.camera, W, H)
    for what, schedule in passes:
        col, bo = pixels(torch, W, H, fmt), pixels(torch, W, H, fmt)
        sc.render(col.ptr, bo.ptr, fmt=fmt, width=W, height=H, schedule=schedule, ss=k)
        torch.cuda.synchronize()
        assert_pair(col, bo, ref, fmt, f"{s.id} ss={k} {W}x{H} fmt {fmt}, {what}")


def check_adaptive(torch, sc, s, fmt=F32, passes=PASSES):
    """Both targets, the mask and the count, as tests/test_gpu_adaptive.py compares them."""
    (W, H), k = S.ADAPTIVE_SIZE.get(s.id, (40, 24)), S.ADAPTIVE_K.get(s.id, 2)
    wc, wb, wm = _adaptive_ref.composed(s.camera, W, H, k, fmt, _adaptive_ref.T, True, s.key)
    sc.camera_uniform = camera_uniform(s.camera, W, H)
    for what, schedule in passes:
        what = f"{s.id} adaptive ss={k} {W}x{H} fmt {fmt}, {what}"
        col, bo = pixels(torch, W, H, fmt), pixels(torch, W, H, fmt)
        mask = torch.full(wm.shape, SENTINEL, dtype=torch.uint8, device="cuda")
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        sc.render(col.ptr, bo.ptr, fmt=fmt, width=W, height=H, schedule=schedule, ss=k, adaptive=_adaptive_ref.T,
                  tile_mask=mask, refined_tiles=count)
        torch.cuda.synchronize()
        gm = mask.cpu().numpy()
        assert np.array_equal(gm, wm), f"{what}: tile_mask got\n{gm}\nwant\n{wm}"
        assert int(count.item()) == int(wm.sum()), f"{what}: refined_tiles"
        assert_frame(col.bytes(), wc, f"{what}: col")
        assert_frame(bo.bytes(), wb, f"{what}: blackout_col")


def check_shutter(torch, sc, s, n, W, H, k=1, fmt=F32, passes=PASSES):
    cams = S.shutter_cameras(s, n, W, H)
    ref = _shutter_ref.reference(cams, W, H, k, s.key)
    for what, schedule in passes:
        col, bo = pixels(torch, W, H, fmt), pixels(torch, W, H, fmt)
        sc.render_shutter(col.ptr, bo.ptr, cameras=list(cams), fmt=fmt, width=W, height=H, ss=k, schedule=schedule or T)
        torch.cuda.synchronize()
        assert_pair(col, bo, ref, fmt, f"{s.id} shutter n={n} ss={k} {W}x{H} fmt {fmt}, {what}")


def lens_records(torch, sc, W, H, schedule, **kw):
    lens = Target(torch, (H, W), 8)
    sc.render_lens(lens.ptr, width=W, height=H, schedule=schedule, **kw)
    torch.cuda.synchronize()
    return lens


def assert_records(lens, want, what):
    got = lens.bytes().view(np.uint32)
    bad = (got != np.ascontiguousarray(want).view(np.uint32)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} records differ, first at {np.argwhere(bad)[:4].tolist()}"


def check_rays(torch, sc, s, dirs, pos, W, H, ref, what, k=1, fmt=F32, dbg=None, passes=PASSES):
    """ref: (col, blackout_col); dbg: (n_rk, fate) of the oracle (ss 1 only)"""
    d = upload(torch, dirs)
    for name, schedule in passes:
        col, bo = pixels(torch, W, H, fmt), pixels(torch, W, H, fmt)
        kw = {}
        if dbg is not None:
            kw = dict(dbg_n_rk=torch.zeros((H, W), dtype=torch.int16, device="cuda"),
                      dbg_fate=torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda"))
        sc.render_rays(d, col.ptr, bo.ptr, pos=pos, fmt=fmt, width=W, height=H, ss=k, schedule=schedule, **kw)
        torch.cuda.synchronize()
        assert_pair(col, bo, ref, fmt, f"{s.id} {what} ss={k} {W}x{H} fmt {fmt}, {name}")
        if dbg is not None:
            for label, got, want in (("fate", kw["dbg_fate"].cpu().numpy(), dbg[1]),
                                     ("n_rk", kw["dbg_n_rk"].cpu().numpy().view(np.uint16), dbg[0])):
                at = np.argwhere(got != want)
                assert not len(at), (f"{s.id} {what}, {name}: {label} differs at {at[:6].tolist()}: got "
                                     f"{got[got != want][:6].tolist()}, want {want[got != want][:6].tolist()}")
    assert np.array_equal(d.cpu().numpy().view(np.uint32), np.ascontiguousarray(dirs).view(np.uint32)), "the map is an input"


# ---- supersampled -------------------------------------------------------------------------------------------------
SS_CASES = ([(sid, W, H, 2) for sid in S.IDS for W, H in S.SIZES] + [(sid, 13, 7, 4) for sid in S.SS_K4] +
            [(sid, 13, 7, 8) for sid in S.SS_K8])


@pytest.mark.parametrize("sid,W,H,k", SS_CASES)
def test_ss(torch_cuda, sid, W, H, k):
    s = S.BY_ID[sid]
    with Scene(s) as sc:
        check_ss(torch_cuda, sc, s, W, H, k)


# ---- adaptive -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", S.ADAPTIVE)
def test_adaptive(torch_cuda, sid):
    s = S.BY_ID[sid]
    with Scene(s) as sc:
        check_adaptive(torch_cuda, sc, s)


# ---- shutter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,W,H", S.SHUTTER_SHAPES)
@pytest.mark.parametrize("sid", S.SHUTTER)
def test_shutter(torch_cuda, sid, n, W, H):
    s = S.BY_ID[sid]
    with Scene(s) as sc:
        check_shutter(torch_cuda, sc, s, n, W, H)


@pytest.mark.parametrize("sid,n,W,H", S.SHUTTER_SS)
def test_shutter_with_ss(torch_cuda, sid, n, W, H):
    s = S.BY_ID[sid]
    with Scene(s) as sc:
        check_shutter(torch_cuda, sc, s, n, W, H, k=2)


# ---- lens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", S.SIZES)
@pytest.mark.parametrize("sid", S.IDS)
def test_lens_and_shade(torch_cuda, sid, W, H):
    """The records as tests/test_gpu_lens.py compares them, in every pass; then the last pass's records shaded with
    the scene's sky and with a sky of another size, against the oracle's frame with that sky."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    want = _lens_ref.records(s.camera, W, H, 1, s.key)[0]
    with Scene(s) as sc:
        sc.camera_uniform = camera_uniform(s.camera, W, H)
        for what, schedule in PASSES:
            lens = lens_records(torch, sc, W, H, schedule)
            assert_records(lens, want, f"{sid} lens {W}x{H}, {what}")
        skies = {"ctx": None, "96x40": bh.Sky(sc, _lens_ref.sky("96x40"))}
        for sky_name, sky in skies.items():
            col, bo = pixels(torch, W, H), pixels(torch, W, H)
            sc.shade(lens.ptr, col.ptr, bo.ptr, sky=sky, width=W, height=H)
            torch.cuda.synchronize()
            assert_pair(col, bo, _lens_ref.frame(s.camera, W, H, sky_name, 1, s.key), F32, f"{sid} shade {sky_name} {W}x{H}")


@pytest.mark.parametrize("sid", S.MIP)
def test_filtered_shade(torch_cuda, sid):
    """The shade has no fold: this checks that the records of the other folds carry what the level selection reads."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    W, H = 40, 24
    wc, wb = shade_mip_np(_lens_ref.records(s.camera, W, H, 1, s.key)[0], "96x40")
    with Scene(s) as sc:
        sc.camera_uniform = camera_uniform(s.camera, W, H)
        lens = lens_records(torch, sc, W, H, 0)
        col, bo = pixels(torch, W, H), pixels(torch, W, H)
        sc.shade(lens.ptr, col.ptr, bo.ptr, sky=bh.Sky(sc, _lens_ref.sky("96x40"), mips=True), width=W, height=H, mip=True)
        torch.cuda.synchronize()
        assert_pair(col, bo, (wc, wb), F32, f"{sid} filtered shade")


# ---- ray maps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", S.SIZES)
@pytest.mark.parametrize("sid", S.IDS)
def test_rays_pinhole(torch_cuda, sid, W, H):
    """The pinhole map of the scenario's camera: the oracle's frame, its n_rk and fate, and Scene.render's own bytes."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    cu = camera_uniform(s.camera, W, H)
    ref = _lens_ref.frame(s.camera, W, H, "ctx", 1, s.key)
    with Scene(s) as sc:
        check_rays(torch, sc, s, _rays_ref.pinhole_map(s.camera, W, H), cu.pos, W, H, ref, "pinhole map",
                   dbg=_rays_ref.oracle_dbg(s.camera, W, H, s.key))
        sc.camera_uniform = cu
        col, bo = pixels(torch, W, H), pixels(torch, W, H)
        sc.render(col.ptr, bo.ptr, width=W, height=H)
        torch.cuda.synchronize()
        assert_pair(col, bo, ref, F32, f"{sid} Scene.render {W}x{H}")


@pytest.mark.parametrize("W,H", S.SIZES)
@pytest.mark.parametrize("name", S.GENERAL_POSITIONS)
@pytest.mark.parametrize("sid", S.GENERAL_MAPS)
def test_rays_general(torch_cuda, sid, name, W, H):
    s = S.BY_ID[sid]
    wc, wb, _, fate, n_rk = _rays_ref.general(name, W, H, s.key)
    with Scene(s) as sc:
        check_rays(torch_cuda, sc, s, _rays_ref.general_map(name, W, H), _rays_ref.position(name), W, H, (wc, wb),
                   f"general map from {name}", dbg=(n_rk, fate))


@pytest.mark.parametrize("sid", S.RAYS_SS)
def test_rays_ss(torch_cuda, sid):
    s = S.BY_ID[sid]
    W, H, k = 13, 7, 2
    with Scene(s) as sc:
        check_rays(torch_cuda, sc, s, _rays_ref.equirect_map(k * W, k * H), _rays_ref.position(s.camera), W, H,
                   _rays_ref.equirect_ss(s.camera, W, H, k, s.key), f"equirect map from {s.camera}", k=k)


@pytest.mark.parametrize("sid", S.LENS_RAYS)
def test_lens_of_a_map(torch_cuda, sid):
    """render_lens(dirs=): the pinhole map at 40x24 gives the camera's records, the general maps at 13x7 theirs."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    cases = [("pinhole map", _rays_ref.pinhole_map(s.camera, 40, 24), camera_uniform(s.camera, 40, 24).pos,
              _lens_ref.records(s.camera, 40, 24, 1, s.key)[0])]
    cases += [(f"general map from {name}", _rays_ref.general_map(name, 13, 7), _rays_ref.position(name),
               _rays_ref.general(name, 13, 7, s.key)[2]) for name in S.GENERAL_POSITIONS]
    with Scene(s) as sc:
        for what, m, pos, want in cases:
            H, W = m.shape[:2]
            d = upload(torch, m)
            for name, schedule in PASSES:
                lens = lens_records(torch, sc, W, H, schedule, dirs=d, pos=pos)
                assert_records(lens, want, f"{sid} lens of the {what}, {name}")


# ---- formats ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F16, BGRA8])
@pytest.mark.parametrize("sid", S.FORMATS)
def test_formats(torch_cuda, sid, fmt):
    """Format and fold are independent template arguments: one scenario per fold and format, in the ss, shutter,
    adaptive and ray-map forms."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    W, H = 40, 24
    with Scene(s) as sc:
        check_ss(torch, sc, s, W, H, 2, fmt)
        check_shutter(torch, sc, s, 4, W, H, fmt=fmt)
        check_adaptive(torch, sc, s, fmt)
        check_rays(torch, sc, s, _rays_ref.pinhole_map(s.camera, W, H), camera_uniform(s.camera, W, H).pos, W, H,
                   _lens_ref.frame(s.camera, W, H, "ctx", 1, s.key), "pinhole map", fmt=fmt)


# ---- posed ray maps and origin maps: every fold and format ----------------------------------------------------------
FOLDS = ["none_F2", "far_off", "disc_F2"]  # Const<0>, Const<BH_SCENE_DEFAULT>, SF_DYN
POSED = ("axesD", "rotH")                  # tests/_rays_pose_ref.py: far outside the unit sphere, and just outside it


def posed_traces(s, k, origins, W=13, H=7):
    """Per pose of POSED: (col, blackout_col, records) of the camera-space map of the virtual frame kW x kH turned by
    the pose -- with `origins`, from the scatter of tests/_rays_origins_ref.py -- resolved when k > 1."""
    kind = "general" if k == 1 else "equirect"
    out = []
    for name in POSED:
        t = (_rays_origins_ref.traced(name, kind, "scatter", k * W, k * H, s.key) if origins
             else _rays_pose_ref.posed(name, kind, k * W, k * H, s.key))
        out.append(t[:3] if k == 1 else (resolve_np(t[0], k), resolve_np(t[1], k), None))
    return kind, out


def check_posed(torch, sc, s, fmt, k, origins, W=13, H=7):
    """render_frames_rays of the two poses in one launch, each frame against its own trace."""
    kind, want = posed_traces(s, k, origins)
    d = upload(torch, _rays_pose_ref.camera_map(kind, k * W, k * H))
    o = upload(torch, _rays_origins_ref.origins("scatter", k * W, k * H)) if origins else None
    for what, schedule in PASSES:
        cols, bos = [pixels(torch, W, H, fmt) for _ in POSED], [pixels(torch, W, H, fmt) for _ in POSED]
        sc.render_frames_rays(d, [t.ptr for t in cols], [t.ptr for t in bos], poses=[_rays_pose_ref.rows(n) for n in POSED],
                              origins=o, fmt=fmt, ss=k, width=W, height=H, schedule=schedule)
        torch.cuda.synchronize()
        for i, name in enumerate(POSED):
            assert_pair(cols[i], bos[i], want[i], fmt,
                        f"{s.id} pose {name}{' with origins' if origins else ''} ss={k} fmt {fmt}, {what}")


def check_shutter_rays(torch, sc, s, fmt, W=13, H=7):
    """render_shutter_rays with the two poses as one exposure: the time tree over their traces."""
    kind, frames = posed_traces(s, 1, False)
    ref = tuple(_shutter_ref.time_tree_np(np.stack([f[t] for f in frames])) for t in (0, 1))
    d = upload(torch, _rays_pose_ref.camera_map(kind, W, H))
    for what, schedule in PASSES:
        col, bo = pixels(torch, W, H, fmt), pixels(torch, W, H, fmt)
        sc.render_shutter_rays(d, col.ptr, bo.ptr, poses=[_rays_pose_ref.rows(n) for n in POSED], fmt=fmt, width=W,
                               height=H, schedule=schedule or T)
        torch.cuda.synchronize()
        assert_pair(col, bo, ref, fmt, f"{s.id} shutter over a posed map fmt {fmt}, {what}")


@pytest.mark.parametrize("fmt", [F32, F16, BGRA8])
@pytest.mark.parametrize("sid", FOLDS)
def test_map_forms_by_fold_and_format(torch_cuda, sid, fmt):
    """Every kernel that the ray-map launchers choose by format, fold and ss, at 13x7: the supersampled ray map, the
    posed map and the posed map with origins, plain and supersampled, and the shutter over a posed map."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    W, H, k = 13, 7, 2
    with Scene(s) as sc:
        check_rays(torch, sc, s, _rays_ref.equirect_map(k * W, k * H), _rays_ref.position("F2"), W, H,
                   _rays_ref.equirect_ss("F2", W, H, k, s.key), "equirect map from F2", k=k, fmt=fmt)
        for origins in (False, True):
            check_posed(torch, sc, s, fmt, 1, origins)
            check_posed(torch, sc, s, fmt, k, origins)
        check_shutter_rays(torch, sc, s, fmt)


@pytest.mark.parametrize("sid", FOLDS)
def test_lens_of_a_posed_map(torch_cuda, sid):
    """render_lens(dirs=, pose=) and render_lens(dirs=, pose=, origins=) at 13x7: the records of the traces."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    W, H = 13, 7
    with Scene(s) as sc:
        for origins in (False, True):
            kind, want = posed_traces(s, 1, origins)
            d = upload(torch, _rays_pose_ref.camera_map(kind, W, H))
            o = upload(torch, _rays_origins_ref.origins("scatter", W, H)) if origins else None
            for i, name in enumerate(POSED):
                for what, schedule in PASSES:
                    lens = lens_records(torch, sc, W, H, schedule, dirs=d, pose=_rays_pose_ref.rows(name), origins=o)
                    assert_records(lens, want[i][2], f"{sid} lens of pose {name}{' with origins' if origins else ''}, {what}")


# ---- several frames in one launch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sid,n", [("disc_F2", 33), ("long_odd", 3)])
@pytest.mark.parametrize("adaptive", [False, True])
def test_multi_frame(torch_cuda, sid, n, adaptive):
    """render_frames(ss=2) and render_frames(ss=2, adaptive=0.1) at 13x7 with the MIXED cameras cycled: 33 frames are
    more than travel in the kernel argument (BH_INLINE_FRAMES = 32), so the epilogue selects its outputs from the
    device table.  Each frame against its own single-frame reference."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    W, H, k = 13, 7, 2
    names = [_shutter_ref.MIXED[i % len(_shutter_ref.MIXED)] for i in range(n)]
    with Scene(s) as sc:
        for what, schedule in PASSES:
            cols, bos = [pixels(torch, W, H) for _ in names], [pixels(torch, W, H) for _ in names]
            kw = {}
            if adaptive:
                kw = dict(adaptive=_adaptive_ref.T, tile_mask=torch.full((n, 1, 2), SENTINEL, dtype=torch.uint8, device="cuda"),
                          refined_tiles=torch.full((n,), -1, dtype=torch.int32, device="cuda"))
            sc.render_frames([t.ptr for t in cols], [t.ptr for t in bos], cameras=[camera_uniform(c, W, H) for c in names],
                             width=W, height=H, ss=k, schedule=schedule, **kw)
            torch.cuda.synchronize()
            for i, cam in enumerate(names):
                tag = f"{sid} frame {i} ({cam}), {what}"
                if adaptive:
                    wc, wb, wm = _adaptive_ref.composed(cam, W, H, k, F32, _adaptive_ref.T, True, s.key)
                    assert np.array_equal(kw["tile_mask"][i].cpu().numpy(), wm), f"{tag}: tile_mask"
                    assert int(kw["refined_tiles"][i].item()) == int(wm.sum()), f"{tag}: refined_tiles"
                    assert_frame(cols[i].bytes(), wc, f"{tag}: col")
                    assert_frame(bos[i].bytes(), wb, f"{tag}: blackout_col")
                else:
                    assert_pair(cols[i], bos[i], reference(cam, W, H, k, s.key), F32, tag)


# ---- the plain kernel as the instrument ---------------------------------------------------------------------------
@pytest.mark.parametrize("sid", S.LONG)
def test_the_fast_forward_fires(torch_cuda, sid):
    """The CPU count of cycling rays (tests/test_scenarios_host.py) compares ro and rd only; the kernel's test also
    compares travelled and outside.  So, on the machine: the plain kernel -- the instrument that
    tests/test_gpu_parity.py::test_cycle_fast_forward_is_exact trusts -- executes fewer steps than n_rk on at least
    one pixel of the scenario's 40x24 frame, and its frame is the oracle's."""
    s = S.BY_ID[sid]
    W, H = 40, 24
    with Scene(s) as sc:
        col, bo, n_rk, fate, steps = gpu_render(torch_cuda, sc, camera_uniform(s.camera, W, H), scenario_uniforms(s.key),
                                                W, H, s.cap, s.flags, bh.BH_MATH_EXACT, steps=True)
    want_n, want_f = _rays_ref.oracle_dbg(s.camera, W, H, s.key)
    assert np.array_equal(n_rk, want_n) and np.array_equal(fate, want_f)
    assert_frame(col.view(np.uint8), _lens_ref.frame(s.camera, W, H, "ctx", 1, s.key)[0], f"{sid} plain col")
    forwarded = steps < n_rk
    print(f"{sid}: the fast-forward fired on {int(forwarded.sum())} pixels")
    assert forwarded.any() and (n_rk[forwarded] == s.cap).all() and (fate[forwarded] == bh.BH_FATE_CAP).all()


# ---- fast math ----------------------------------------------------------------------------------------------------
def fast_plain(torch, sc, cu, W, H):
    """(col, blackout_col) fp32 (H, W, 4) of the fast-math plain render"""
    sc.camera_uniform = cu
    col, bo = pixels(torch, W, H), pixels(torch, W, H)
    sc.render(col.ptr, bo.ptr, width=W, height=H)
    torch.cuda.synchronize()
    out = col.bytes().view(np.float32).reshape(H, W, 4), bo.bytes().view(np.float32).reshape(H, W, 4)
    assert not np.isnan(out[0]).any() and not np.isnan(out[1]).any()
    return out


def assert_fast(got, want, what):
    """bit-equal to the composition, after printing how far it is"""
    for name, g, w in (("col", got[0], want[0]), ("blackout_col", got[1], want[1])):
        g = g.bytes().view(np.float32).reshape(w.shape)
        differ = int((g.view(np.uint32) != w.view(np.uint32)).any(-1).sum())
        delta = float(np.abs(g - w).max())
        print(f"{what} {name}: {differ} of {g.shape[0] * g.shape[1]} pixels differ in bits, max |delta| {delta:.3e}")
        assert delta < FAST_TOL, f"{what} {name}: outside the fast tolerance"
        assert (g[..., 3] == 1.0).all()
        assert_frame(g.view(np.uint8), w, f"{what} {name}")


@pytest.mark.parametrize("sid", S.FAST)
def test_fast_math_ss_by_composition(torch_cuda, sid):
    """BH_MATH_FAST has no bit-exact oracle, so it is checked by composition (the project's rule,
    tests/test_gpu_ss.py::test_fast_math_by_composition): ss = 2 in fast math is bit-equal to the numpy tree over the
    GPU's own fast-math plain render of the virtual frame -- here in the fast build's SF_DYN kernels."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    W, H, k = 40, 24, 2
    with Scene(s, bh.BH_MATH_FAST) as sc:
        vc, vb = fast_plain(torch, sc, camera_uniform(s.camera, W, H), k * W, k * H)
        col, bo = pixels(torch, W, H), pixels(torch, W, H)
        sc.render(col.ptr, bo.ptr, width=W, height=H, ss=k)
        torch.cuda.synchronize()
        assert_fast((col, bo), (resolve_np(vc, k), resolve_np(vb, k)), f"{sid} fast ss={k}")


@pytest.mark.parametrize("sid", S.FAST)
def test_fast_math_shutter_by_composition(torch_cuda, sid):
    """The shutter render in fast math is bit-equal to the numpy time tree over the GPU's own fast-math plain frames
    of the same cameras (tests/test_gpu_shutter.py::test_fast_math_by_composition)."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    W, H, n = 40, 24, 4
    cams = S.shutter_cameras(s, n, W, H)
    with Scene(s, bh.BH_MATH_FAST) as sc:
        frames = [fast_plain(torch, sc, cu, W, H) for cu in cams]
        col, bo = pixels(torch, W, H), pixels(torch, W, H)
        sc.render_shutter(col.ptr, bo.ptr, cameras=list(cams), width=W, height=H)
        torch.cuda.synchronize()
        want = tuple(_shutter_ref.time_tree_np(np.stack([f[t] for f in frames])) for t in (0, 1))
        assert_fast((col, bo), want, f"{sid} fast shutter n={n}")


@pytest.mark.parametrize("sid", S.FAST)
def test_fast_math_adaptive_by_composition(torch_cuda, sid):
    """The adaptive render in fast math (tests/test_gpu_adaptive.py::test_fast_math_by_composition): the mask is the
    numpy rule over the GPU's fast plain frame, unrefined pixels are that frame's bytes, refined pixels are within
    FAST_TOL of the GPU's fast ss render (bit equality is printed, not required: the fast build's contraction depends
    on the surrounding code)."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    (W, H), k = S.ADAPTIVE_SIZE.get(sid, (40, 24)), S.ADAPTIVE_K.get(sid, 2)
    with Scene(s, bh.BH_MATH_FAST) as sc:
        pc, pb = fast_plain(torch, sc, camera_uniform(s.camera, W, H), W, H)
        sc_, sb = pixels(torch, W, H), pixels(torch, W, H)
        sc.render(sc_.ptr, sb.ptr, width=W, height=H, ss=k)
        col, bo = pixels(torch, W, H), pixels(torch, W, H)
        wm = _adaptive_ref.tile_mask(F32, pc, pb, _adaptive_ref.T)
        assert 0 < int(wm.sum()) < wm.size
        mask = torch.full(wm.shape, SENTINEL, dtype=torch.uint8, device="cuda")
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        sc.render(col.ptr, bo.ptr, width=W, height=H, ss=k, adaptive=_adaptive_ref.T, tile_mask=mask, refined_tiles=count)
        torch.cuda.synchronize()
        assert np.array_equal(mask.cpu().numpy(), wm) and int(count.item()) == int(wm.sum())
        pm = _adaptive_ref.pixel_mask(wm, W, H)
        for name, g, p, q in (("col", col, pc, sc_), ("blackout_col", bo, pb, sb)):
            g = g.bytes().view(np.float32).reshape(H, W, 4)
            q = q.bytes().view(np.float32).reshape(H, W, 4)
            assert np.array_equal(g[~pm].view(np.uint32), p[~pm].view(np.uint32)), f"{sid} {name}: unrefined pixels"
            differ = int((g[pm].view(np.uint32) != q[pm].view(np.uint32)).any(-1).sum())
            delta = float(np.abs(g[pm] - q[pm]).max())
            print(f"{sid} fast adaptive ss={k} {name}: {differ} of {int(pm.sum())} refined pixels differ in bits from the "
                  f"fast ss render, max |delta| {delta:.3e}")
            assert delta < FAST_TOL, f"{sid} {name}: refined pixels"
