"""BH_MATH_FAST in every form the launchers reach.  The fast build (csrc/bh_march_fast.hip) is a second, complete
build of the march -- its own ops, its own arms of the step, every kernel in three formats -- of which the rest of
the suite runs the tile schedule, RGBA32F, row-major, one frame per launch.  Here:

  1. every schedule against the f64 frame, under the allowance of tests/_f64_ref.py (the references' own
     sensitivity to one ulp; tests/test_f64_ref_host.py shows that the rule holds the references and has teeth);
  2. what is a run-time argument of one kernel instance -- layout, shard, partition, frame count, stream, a missing
     target -- gives that instance's row-major bytes, with no allowance;
  3. the RGBA16F and BGRA8 instantiations against the encode of their schedule's own fp32 fast frame;
  4. the supersampled, shutter and adaptive forms in RGBA16F and BGRA8 against the numpy composition of the GPU's
     own fast fp32 frames;
  6. frames of 1 to 7 tiles under every schedule, in both math modes.
(5, the input edges under every schedule, is tests/test_gpu_edge_inputs.py's.)

Every target is pre-filled with bytes no render writes.  Tests that measure print their figures (pytest -s)."""
import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from oracle import oracle_np
from tests import _adaptive_ref, _f64_ref, _shutter_ref
from tests import _scenarios as S
from tests._cases import camera_uniform, uniforms
from tests._gpu_common import FAST_TOL, SCHEDULES, assert_bitexact, oracle_render
from tests._ss_ref import expected_bytes, resolve_np, scenario_uniforms

pytestmark = pytest.mark.gpu

F32, F16, BGRA8 = bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB
FORMATS = [F32, F16, BGRA8]
FMT_IDS = ["rgba32f", "rgba16f", "bgra8"]
NP_DT = {F32: np.float32, F16: np.float16, BGRA8: np.uint8}
TILE, PAIR, PERSISTENT = bh.BH_SCHED_TILE, bh.BH_SCHED_PAIR, bh.BH_SCHED_PERSISTENT
STATIC = TILE | bh.BH_SCHED_FLAG_STATIC_ORDER
SENTINEL = 0xA5   # every byte of a target before a render: as fp32 / fp16 no value a frame holds, as a fate 165


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def filled(torch, nbytes):
    return torch.full((int(nbytes),), SENTINEL, dtype=torch.uint8, device="cuda")


def frame_of(buf, fmt, H, W):
    return buf.cpu().numpy().view(NP_DT[fmt]).reshape(H, W, 4)


def render(torch, scene, cu, W, H, fmt=F32, schedule=TILE, blackout=True, dbg=True, math=bh.BH_MATH_FAST, stream=None):
    """One row-major render into sentinel-filled targets: (col, blackout_col or None, n_rk or None, fate or None)."""
    scene.camera_uniform = cu
    bpp = _abi.BYTES_PER_PIXEL[fmt]
    col = filled(torch, W * H * bpp)
    bo = filled(torch, W * H * bpp) if blackout else None
    nrk = filled(torch, W * H * 2) if dbg else None
    fate = filled(torch, W * H) if dbg else None
    scene.render(col, bo, fmt=fmt, math=math, dbg_n_rk=nrk, dbg_fate=fate, width=W, height=H, schedule=schedule,
                 stream=stream)
    torch.cuda.synchronize()
    return (frame_of(col, fmt, H, W), None if bo is None else frame_of(bo, fmt, H, W),
            None if nrk is None else nrk.cpu().numpy().view(np.uint16).reshape(H, W),
            None if fate is None else fate.cpu().numpy().reshape(H, W))


def blackout_of(col):
    """blackout_col as the per-pixel function of an fp32 col (src/black_hole_maybe.wgsl:365-368)."""
    keep = ~(((col[..., 0] * col[..., 0] + col[..., 1] * col[..., 1]) + col[..., 2] * col[..., 2]) < 1.0)
    return np.where(keep[..., None], col, np.array([0, 0, 0, 1], np.float32))


def assert_valid(g, cap):
    col, bo, nrk, fate = g
    assert fate.max() <= 3, np.unique(fate)
    assert int(nrk.max()) <= cap
    assert np.isfinite(col).all() and (col[..., 3] == 1).all()
    assert (col[..., :3] >= 0).all() and (col[..., :3] <= 1).all()
    assert np.array_equal(bo.view(np.uint32), blackout_of(col).view(np.uint32)), "blackout_col is not the function of col"


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8).ravel(), np.ascontiguousarray(b).view(np.uint8).ravel())


def bits_differ(a, b):
    """pixels on which two frames of one format differ in any bit"""
    n = a.shape[-1] * a.dtype.itemsize
    return (np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[:2] + (n,))
            != np.ascontiguousarray(b).view(np.uint8).reshape(b.shape[:2] + (n,))).any(-1)


def decoded(fmt, x):
    """the linear fp64 RGB that the stored texels x of format fmt stand for"""
    if fmt == BGRA8:
        return oracle_np.srgb_lut().astype(np.float64)[x[..., 2::-1]]
    return x[..., :3].astype(np.float64)


# ---- 1. schedules against f64 -------------------------------------------------------------------------------------
SCHED1 = [("tile", TILE), ("tile_learned", TILE), ("tile_static", STATIC), ("pair", PAIR), ("persistent", PERSISTENT)]
SCHED1_IDS = [s[0] for s in SCHED1]
_frames = {}


def fast_frames(torch, sky, case_id):
    """The case's fast fp32 frame under each schedule of SCHED1, rendered once per session in a fresh Scene (so the
    first tile frame runs the order of a fresh state and the second the learned one)."""
    if case_id not in _frames:
        cam, W, H, cap, flags, over = _f64_ref.CASES[case_id]
        scene = bh.Scene(16, 16, sky=sky, max_iters=cap, scene_flags=flags, math=bh.BH_MATH_FAST)
        scene.uniforms = uniforms(**over)
        cu = camera_uniform(cam, W, H)
        _frames[case_id] = {name: render(torch, scene, cu, W, H, schedule=sched) for name, sched in SCHED1}
        scene.close()
    return _frames[case_id]


@pytest.mark.parametrize("name", SCHED1_IDS)
@pytest.mark.parametrize("case_id", _f64_ref.CASE_IDS)
def test_schedules_against_f64(torch_cuda, sky_small, case_id, name):
    """d(F) <= allowance = 2 max(d(E), d(N_0..7)) + 2 against the f64 frame (tests/_f64_ref.py), valid outputs, and
    blackout_col the per-pixel function of col bit for bit.
    Measured on an MI355X: DESIGN.md §3 "Parity bar" holds the table of d(F), y and allowance per case and schedule."""
    ref = _f64_ref.reference(case_id, sky_small)
    frames = fast_frames(torch_cuda, sky_small, case_id)
    g = frames[name]
    dF = ref.d((g[0], g[2], g[3]))
    vs_tile = int((bits_differ(g[0], frames["tile"][0]) | (g[2] != frames["tile"][2]) | (g[3] != frames["tile"][3])).sum())
    print(f"F64RULE {case_id} {name}: d(F) {dF}, y {ref.y}, allowance {ref.allowance}, d(E) {ref.d_E}, "
          f"{vs_tile} pixels differ in bits from the tile frame")
    assert_valid(g, ref.cap)
    assert dF <= ref.allowance, f"d(F) {dF} > allowance {ref.allowance} (y {ref.y})"


@pytest.mark.parametrize("case_id", _f64_ref.CASE_IDS)
def test_tile_orders_are_byte_equal(torch_cuda, sky_small, case_id):
    """The learned order and the static order change no byte of the fresh order's frame."""
    frames = fast_frames(torch_cuda, sky_small, case_id)
    for name in ("tile_learned", "tile_static"):
        for k in range(4):
            assert same_bytes(frames[name][k], frames["tile"][k]), (name, k)


@pytest.mark.parametrize("case_id", _f64_ref.CASE_IDS)
def test_schedules_agree_pairwise(torch_cuda, sky_small, case_id):
    """Two schedules are two kernels (march_step / march_step2, other contraction): their frames may differ where a
    trajectory does, by the three criteria of d() and within the same allowance."""
    ref = _f64_ref.reference(case_id, sky_small)
    frames = fast_frames(torch_cuda, sky_small, case_id)
    names = ["tile", "pair", "persistent"]
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            a, b = frames[p], frames[q]
            n = _f64_ref.d((a[0], a[2], a[3]), (b[0], b[2], b[3]))
            print(f"F64PAIR {case_id} {p} vs {q}: {n} pixels disagree, allowance {ref.allowance}")
            assert n <= ref.allowance, f"{p} vs {q}: {n} > {ref.allowance}"


# ---- 2. same kernel, same bits ------------------------------------------------------------------------------------
W2, H2, CAP2 = _f64_ref.W, _f64_ref.H, 512
SCHED2 = [("tile", TILE), ("pair", PAIR), ("persistent", PERSISTENT)]
SCHED2_IDS = [s[0] for s in SCHED2]


@pytest.fixture(scope="module")
def scene_d(torch_cuda, sky_small):
    scene = bh.Scene(W2, H2, sky=sky_small, max_iters=CAP2, math=bh.BH_MATH_FAST)
    scene.camera_uniform = camera_uniform("D", W2, H2)
    yield scene
    scene.close()


@pytest.fixture(scope="module")
def rowmajor_d(torch_cuda, scene_d):
    """(col, blackout_col, n_rk, fate) of camera D per (schedule, format): the fast row-major frame that every other
    transport of that kernel instance must reproduce.  Rendered once, read-only."""
    cache = {}

    def get(schedule, fmt, cam="D"):
        key = (schedule, fmt, cam)
        if key not in cache:
            g = render(torch_cuda, scene_d, camera_uniform(cam, W2, H2), W2, H2, fmt=fmt, schedule=schedule)
            for a in g:
                a.setflags(write=False)
            cache[key] = g
        scene_d.camera_uniform = camera_uniform("D", W2, H2)
        return cache[key]
    return get


def _shards(torch, scene, layout, fmt, S, schedule, both, partition=None):
    """Every shard of camera D's frame in a BH_LAYOUT_TILES* layout, as the gather concatenates them:
    (packed col, packed blackout_col or None, stride in tiles)."""
    tb = bh.tile_bytes(layout, fmt)
    counts = partition.counts if partition else [bh.shard_tile_count(W2, H2, k, S) for k in range(S)]
    assert sum(counts) == ((W2 + 7) // 8) * ((H2 + 7) // 8)
    stride = max(counts)
    pc = filled(torch, S * stride * tb).view(S * stride, tb)
    pb = filled(torch, S * stride * tb).view(S * stride, tb) if both else None
    kw = dict(partition=partition) if partition else {}
    for k in range(S):
        if counts[k] == 0:   # a weight-0 rank renders nothing
            continue
        sl = slice(k * stride, k * stride + counts[k])
        scene.render(pc[sl], pb[sl] if both else None, fmt=fmt, layout=layout, shard_index=k, shard_count=S,
                     width=W2, height=H2, schedule=schedule, **kw)
    return pc, pb, stride


def _out(torch, fmt):
    return filled(torch, W2 * H2 * _abi.BYTES_PER_PIXEL[fmt])


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name,schedule", SCHED2, ids=SCHED2_IDS)
def test_tiles_and_tiles_rgb_shards_unpack(torch_cuda, scene_d, rowmajor_d, name, schedule, fmt, S):
    """BH_LAYOUT_TILES through bh_tiles_unpack and BH_LAYOUT_TILES_RGB through bh_tiles_unpack_rgb (all rows at once
    and two in flight): both targets, every shard count, equal to the schedule's row-major frame byte for byte."""
    torch = torch_cuda
    want_c, want_b = rowmajor_d(schedule, fmt)[:2]
    bpp = _abi.BYTES_PER_PIXEL[fmt]
    pc, pb, stride = _shards(torch, scene_d, bh.BH_LAYOUT_TILES, fmt, S, schedule, True)
    for packed, want, what in ((pc, want_c, "col"), (pb, want_b, "blackout_col")):
        out = _out(torch, fmt)
        bh.tiles_unpack(packed, out, W2, H2, S, stride, bpp)
        torch.cuda.synchronize()
        assert same_bytes(frame_of(out, fmt, H2, W2), want), f"tiles {what}"
    pc, pb, stride = _shards(torch, scene_d, bh.BH_LAYOUT_TILES_RGB, fmt, S, schedule, True)
    for rows in (0, 2):
        for packed, want, what in ((pc, want_c, "col"), (pb, want_b, "blackout_col")):
            out = _out(torch, fmt)
            bh.tiles_unpack_rgb(packed, out, W2, H2, S, stride, fmt, rows_in_flight=rows)
            torch.cuda.synchronize()
            assert same_bytes(frame_of(out, fmt, H2, W2), want), f"tiles_rgb {what}, rows_in_flight {rows}"


RGBM = [(bh.BH_LAYOUT_TILES_RGBM, F32, 0), (bh.BH_LAYOUT_TILES_RGBM, F16, 0), (bh.BH_LAYOUT_TILES_RGBM, BGRA8, 0),
        (bh.BH_LAYOUT_TILES_RGBM14, F16, bh.BH_UNPACK_RGBM14)]
RGBM_IDS = ["rgbm_rgba32f", "rgbm_rgba16f", "rgbm_bgra8", "rgbm14_rgba16f"]


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("layout,fmt,unpack", RGBM, ids=RGBM_IDS)
@pytest.mark.parametrize("name,schedule", SCHED2[:2], ids=SCHED2_IDS[:2])   # the RGBM layouts refuse PERSISTENT
def test_rgbm_shards_restore_both_targets(torch_cuda, scene_d, rowmajor_d, name, schedule, layout, fmt, unpack, S):
    """The shards carry col alone (RGB planes and the per-tile blackout mask); bh_tiles_unpack_rgbm restores col and
    blackout_col, equal to the schedule's two-target row-major render byte for byte."""
    torch = torch_cuda
    want_c, want_b = rowmajor_d(schedule, fmt)[:2]
    pc, _, stride = _shards(torch, scene_d, layout, fmt, S, schedule, False)
    out_c, out_b = _out(torch, fmt), _out(torch, fmt)
    bh.tiles_unpack_rgbm(pc, out_c, out_b, W2, H2, S, stride, fmt | unpack)
    torch.cuda.synchronize()
    assert same_bytes(frame_of(out_c, fmt, H2, W2), want_c), "col"
    assert same_bytes(frame_of(out_b, fmt, H2, W2), want_b), "blackout_col"


@pytest.mark.parametrize("layout,fmt,unpack", RGBM, ids=RGBM_IDS)
def test_rgbm_partition_shards_restore_both_targets(torch_cuda, scene_d, rowmajor_d, layout, fmt, unpack):
    """A weighted partition with a rank of weight 0, through bh_tiles_unpack_rgbm_partition (a partition is bound to
    the tile schedule), twice: the second launch runs the learned order of the partition's shards."""
    torch = torch_cuda
    want_c, want_b = rowmajor_d(TILE, fmt)[:2]
    part = bh.Partition(W2, H2, [0, 5, 7])
    for rep in range(2):
        pc, _, stride = _shards(torch, scene_d, layout, fmt, 3, TILE, False, part)
        out_c, out_b = _out(torch, fmt), _out(torch, fmt)
        bh.tiles_unpack_rgbm_partition(pc, out_c, out_b, part, stride, fmt | unpack)
        torch.cuda.synchronize()
        assert same_bytes(frame_of(out_c, fmt, H2, W2), want_c), f"col, launch {rep}"
        assert same_bytes(frame_of(out_b, fmt, H2, W2), want_b), f"blackout_col, launch {rep}"
    part.close()


FRAME_CAMS = ["D", "A", "B", "C", "E"]


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name,schedule,n", [("tile", TILE, 2), ("tile", TILE, 5), ("tile", TILE, 33), ("pair", PAIR, 2),
                                             ("persistent", PERSISTENT, 2)],
                         ids=["tile-2", "tile-5", "tile-33", "pair-2", "persistent-2"])
def test_render_frames_equals_single_renders(torch_cuda, scene_d, rowmajor_d, name, schedule, n, fmt):
    """n frames of different cameras in one bh_render_frames call -- the tile schedule interleaves them in one grid,
    33 of them through the device frame table; the other schedules run n launches -- each frame's targets and debug
    counters equal to its single render, twice (the second tile launch runs the order learned from frame 0)."""
    torch = torch_cuda
    names = [FRAME_CAMS[i % len(FRAME_CAMS)] for i in range(n)]
    cams = [camera_uniform(c, W2, H2) for c in names]
    singles = {c: rowmajor_d(schedule, fmt, c) for c in set(names)}
    bpp = _abi.BYTES_PER_PIXEL[fmt]
    for rep in range(2):
        cols = [filled(torch, W2 * H2 * bpp) for _ in cams]
        bos = [filled(torch, W2 * H2 * bpp) for _ in cams]
        nrks = [filled(torch, W2 * H2 * 2) for _ in cams]
        fates = [filled(torch, W2 * H2) for _ in cams]
        scene_d.render_frames(cols, bos, cameras=cams, fmt=fmt, dbg_n_rk=nrks, dbg_fate=fates, width=W2, height=H2,
                              schedule=schedule)
        torch.cuda.synchronize()
        for i, c in enumerate(names):
            wc, wb, wn, wf = singles[c]
            tag = f"launch {rep}, frame {i} (camera {c})"
            assert same_bytes(frame_of(cols[i], fmt, H2, W2), wc), f"{tag}: col"
            assert same_bytes(frame_of(bos[i], fmt, H2, W2), wb), f"{tag}: blackout_col"
            assert same_bytes(nrks[i].cpu().numpy(), wn), f"{tag}: n_rk"
            assert same_bytes(fates[i].cpu().numpy(), wf), f"{tag}: fate"


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("name,schedule", SCHED2, ids=SCHED2_IDS)
def test_missing_targets_change_no_byte(torch_cuda, scene_d, rowmajor_d, name, schedule, fmt):
    """blackout_col = None, and no dbg_* target, are run-time arguments: col (and blackout_col) stay what they are."""
    want_c, want_b = rowmajor_d(schedule, fmt)[:2]
    cu = camera_uniform("D", W2, H2)
    g = render(torch_cuda, scene_d, cu, W2, H2, fmt=fmt, schedule=schedule, blackout=False)
    assert same_bytes(g[0], want_c), "blackout=None: col"
    g = render(torch_cuda, scene_d, cu, W2, H2, fmt=fmt, schedule=schedule, dbg=False)
    assert same_bytes(g[0], want_c) and same_bytes(g[1], want_b), "no dbg targets"


@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_two_streams_give_the_static_order_frame(torch_cuda, scene_d, rowmajor_d, fmt):
    """Renders interleaved on two streams keep separate order states and give the static order's bytes."""
    torch = torch_cuda
    want_c = rowmajor_d(STATIC, fmt)[0]
    assert same_bytes(want_c, rowmajor_d(TILE, fmt)[0])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = [_out(torch, fmt) for _ in range(6)]
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        scene_d.render(o, None, fmt=fmt, width=W2, height=H2, stream=streams[i % 2])
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert same_bytes(frame_of(o, fmt, H2, W2), want_c), f"render {i}"


# ---- 3. formats ---------------------------------------------------------------------------------------------------
def compare_encoded(fmt, got, want32, allowance, what, evidence=None):
    """The comparator of the format tests.  `got`: stored texels of format fmt; `want32`: the fp32 frame they should
    encode.  Prints and returns the number of differing pixels; requires it to be <= allowance, and every differing
    pixel to decode to within FAST_TOL of the expectation unless `evidence` (a mask: the two renders' own fate or
    n_rk differ there) shows its trajectory to be another one.  Without evidence (a form without dbg targets) nothing
    excuses a pixel: every differing one decodes to within FAST_TOL."""
    want = np.ascontiguousarray(expected_bytes(fmt, want32)).view(NP_DT[fmt]).reshape(got.shape)
    differ = bits_differ(got, want)
    delta = np.abs(decoded(fmt, got) - decoded(fmt, want)).max(-1)
    beyond = differ & ~(delta < FAST_TOL)
    n = int(differ.sum())
    print(f"FMTDIFF {what}: {n} of {differ.size} pixels differ, {int(beyond.sum())} of them by >= {FAST_TOL}, "
          f"max |delta| {float(delta.max()):.3e}, allowance {allowance}")
    assert n <= allowance, f"{what}: {n} pixels differ > allowance {allowance}"
    unexplained = beyond if evidence is None else beyond & ~evidence
    assert not unexplained.any(), (f"{what}: beyond FAST_TOL with no other fate or n_rk to show for it at "
                                   f"{np.argwhere(unexplained)[:4].tolist()}")
    return n


@pytest.mark.parametrize("name,schedule", SCHED2, ids=SCHED2_IDS)
@pytest.mark.parametrize("case_id", _f64_ref.CASE_IDS)
def test_formats_encode_the_fp32_fast_frame(torch_cuda, sky_small, case_id, name, schedule):
    """Each format is its own instantiation of the fast kernels, so the compiler may contract it differently: the
    RGBA16F and BGRA8 frames against astype(float16) and the normative sRGB encode of that schedule's own fp32 fast
    frame.  Measured on an MI355X: DESIGN.md §3 "Parity bar"."""
    ref = _f64_ref.reference(case_id, sky_small)
    cam, W, H, cap, flags, over = _f64_ref.CASES[case_id]
    g32 = fast_frames(torch_cuda, sky_small, case_id)[name]
    scene = bh.Scene(16, 16, sky=sky_small, max_iters=cap, scene_flags=flags, math=bh.BH_MATH_FAST)
    scene.uniforms = uniforms(**over)
    try:
        for fmt, fid in ((F16, "rgba16f"), (BGRA8, "bgra8")):
            g = render(torch_cuda, scene, camera_uniform(cam, W, H), W, H, fmt=fmt, schedule=schedule)
            assert g[3].max() <= 3 and int(g[2].max()) <= cap
            evidence = (g[2] != g32[2]) | (g[3] != g32[3])
            print(f"FMTDBG {case_id} {name} {fid}: fate or n_rk differ from the fp32 render on {int(evidence.sum())} pixels")
            compare_encoded(fmt, g[0], g32[0], ref.allowance, f"{case_id} {name} {fid} col", evidence)
            compare_encoded(fmt, g[1], g32[1], ref.allowance, f"{case_id} {name} {fid} blackout_col", evidence)
    finally:
        scene.close()


# ---- 4. derived forms in the other formats ------------------------------------------------------------------------
W4, H4, K4 = 40, 24, 2


class FastScene:
    """A fresh fast-math Scene of a scenario of tests/_scenarios.py under the suite's small sky."""

    def __init__(self, s, sky):
        self.s, self.sky = s, sky

    def __enter__(self):
        self.sc = bh.Scene(16, 16, sky=self.sky, max_iters=self.s.cap, scene_flags=self.s.flags, math=bh.BH_MATH_FAST)
        self.sc.uniforms = scenario_uniforms(self.s.key)
        return self.sc

    def __exit__(self, *exc):
        self.sc.close()


def form_allowance(s, sky, frames):
    """The allowance of a derived form: the sum over the fast frames it is composed of -- (camera uniform, w, h) each
    -- of that frame's own allowance: an output pixel may differ where any of its samples' trajectories does."""
    U = scenario_uniforms(s.key)
    return sum(_f64_ref.reference_of(cu, U, w, h, s.cap, s.flags, sky).allowance for cu, w, h in frames)


def store(torch, sc, fmt, **kw):
    """(col, blackout_col) of a derived render of W4 x H4 in format fmt"""
    bpp = _abi.BYTES_PER_PIXEL[fmt]
    col, bo = filled(torch, W4 * H4 * bpp), filled(torch, W4 * H4 * bpp)
    call = kw.pop("call", sc.render)
    call(col, bo, fmt=fmt, width=W4, height=H4, **kw)
    torch.cuda.synchronize()
    return frame_of(col, fmt, H4, W4), frame_of(bo, fmt, H4, W4)


@pytest.mark.parametrize("fmt", [F16, BGRA8], ids=FMT_IDS[1:])
@pytest.mark.parametrize("sid", S.FAST)
def test_ss_in_the_other_formats(torch_cuda, sky_small, sid, fmt):
    """ss = 2 in RGBA16F / BGRA8 against the numpy tree over the GPU's own fast fp32 render of the virtual frame."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    cu = camera_uniform(s.camera, W4, H4)
    allowance = form_allowance(s, sky_small, [(cu, K4 * W4, K4 * H4)])
    with FastScene(s, sky_small) as sc:
        vc, vb = render(torch, sc, cu, K4 * W4, K4 * H4, dbg=False)[:2]
        sc.camera_uniform = cu
        col, bo = store(torch, sc, fmt, ss=K4)
    compare_encoded(fmt, col, resolve_np(vc, K4), allowance, f"{sid} ss={K4} fmt {fmt} col")
    compare_encoded(fmt, bo, resolve_np(vb, K4), allowance, f"{sid} ss={K4} fmt {fmt} blackout_col")


@pytest.mark.parametrize("fmt", [F16, BGRA8], ids=FMT_IDS[1:])
@pytest.mark.parametrize("sid", S.FAST)
def test_shutter_in_the_other_formats(torch_cuda, sky_small, sid, fmt):
    """A shutter of n = 2 cameras against the numpy time tree over the GPU's own fast fp32 frames of those cameras."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    cams = S.shutter_cameras(s, 2, W4, H4)
    allowance = form_allowance(s, sky_small, [(cu, W4, H4) for cu in cams])
    with FastScene(s, sky_small) as sc:
        frames = [render(torch, sc, cu, W4, H4, dbg=False)[:2] for cu in cams]
        col, bo = store(torch, sc, fmt, call=sc.render_shutter, cameras=list(cams))
    for t, (got, what) in enumerate(((col, "col"), (bo, "blackout_col"))):
        want = _shutter_ref.time_tree_np(np.stack([f[t] for f in frames]))
        compare_encoded(fmt, got, want, allowance, f"{sid} shutter n=2 fmt {fmt} {what}")


@pytest.mark.parametrize("fmt", [F16, BGRA8], ids=FMT_IDS[1:])
@pytest.mark.parametrize("sid", S.FAST)
def test_adaptive_in_the_other_formats(torch_cuda, sky_small, sid, fmt):
    """The adaptive render (k = 2, the T of tests/_adaptive_ref.py) against where(mask, ss, plain): the encodes of the
    GPU's own fast fp32 plain frame and of the numpy tree over its fast fp32 virtual frame, the mask by the numpy rule
    over the encoded plain frame."""
    torch = torch_cuda
    s = S.BY_ID[sid]
    cu = camera_uniform(s.camera, W4, H4)
    allowance = form_allowance(s, sky_small, [(cu, W4, H4), (cu, K4 * W4, K4 * H4)])
    with FastScene(s, sky_small) as sc:
        pc, pb = render(torch, sc, cu, W4, H4, dbg=False)[:2]
        vc, vb = render(torch, sc, cu, K4 * W4, K4 * H4, dbg=False)[:2]
        sc.camera_uniform = cu
        col, bo = store(torch, sc, fmt, ss=K4, adaptive=_adaptive_ref.T)
    spc, spb = _adaptive_ref.stored(fmt, pc), _adaptive_ref.stored(fmt, pb)
    wm = _adaptive_ref.tile_mask(fmt, spc, spb, _adaptive_ref.T)
    assert 0 < int(wm.sum()) < wm.size
    pm = _adaptive_ref.pixel_mask(wm, W4, H4)[..., None]
    for got, plain, virt, what in ((col, pc, vc, "col"), (bo, pb, vb, "blackout_col")):
        want = np.where(pm, resolve_np(virt, K4), plain)
        compare_encoded(fmt, got, want, allowance, f"{sid} adaptive ss={K4} fmt {fmt} {what}")


# ---- 6. tiny frames, both math modes ------------------------------------------------------------------------------
TINY = [(1, 1), (8, 8), (9, 7), (17, 1), (24, 8), (56, 8)]   # 1, 1, 2, 3, 3 and 7 tiles
TINY_SCHEDULES = SCHEDULES + [TILE]
TINY_SCHED_IDS = ["pair", "tile_issue", "tile_latency", "persistent", "tile"]
CAP6 = 512


@pytest.fixture(scope="module")
def tiny_oracle(sky_small):
    cache = {}

    def get(W, H):
        if (W, H) not in cache:
            o = oracle_render(camera_uniform("A", W, H), uniforms(), sky_small, W, H, CAP6, 3)
            for a in o:
                a.setflags(write=False)
            cache[(W, H)] = o
        return cache[(W, H)]
    return get


@pytest.fixture(scope="module")
def scene_tiny(torch_cuda, sky_small):
    scene = bh.Scene(16, 16, sky=sky_small, max_iters=CAP6)
    yield scene
    scene.close()


@pytest.mark.parametrize("schedule", TINY_SCHEDULES, ids=TINY_SCHED_IDS)
@pytest.mark.parametrize("W,H", TINY, ids=[f"{w}x{h}" for w, h in TINY])
def test_tiny_frames(torch_cuda, scene_tiny, tiny_oracle, W, H, schedule):
    """Fewer tiles than the persistent kernel has work queues (8), and the pair kernel's lone last tile: camera A
    (not grazing), twice per mode (the second tile render runs the learned order).  Exact math is the oracle's bits;
    fast math gives valid outputs with the oracle's fate and n_rk on all but at most 2 pixels.  That bound of 2 is
    the suite's usual one and says nothing on the 1x1 frame and little on 8x8: what holds the smallest sizes is the
    exact mode's bit equality and the validity of the fast outputs (a fate in 0..3, n_rk <= cap, finite colours in
    [0, 1], alpha 1, blackout_col the function of col)."""
    o = tiny_oracle(W, H)
    cu = camera_uniform("A", W, H)
    scene_tiny.uniforms = uniforms()
    for rep in range(2):
        g = render(torch_cuda, scene_tiny, cu, W, H, schedule=schedule, math=bh.BH_MATH_EXACT)
        assert_bitexact(g, o)
        g = render(torch_cuda, scene_tiny, cu, W, H, schedule=schedule, math=bh.BH_MATH_FAST)
        assert_valid(g, CAP6)
        differ = int(((g[2] != o[2]) | (g[3] != o[3])).sum())
        assert differ <= 2, f"render {rep}: fate or n_rk differ from the oracle on {differ} of {W * H} pixels"
