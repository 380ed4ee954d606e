"""The start of a march wave on the GPU (bh_march_tile.hpp: slot_head, march_tile_wave, srgb_fetch / srgb_store):
the table copy by one 16-byte load per lane, the slot's chain on the scalar unit -- slot / n_frames and tile /
tiles_x by the host's magics, the order entry, the tile list's, the frame's record from the kernel argument or the
device table -- and the camera in SGPRs.  None of it may change a byte: every case is compared bit for bit with the
CPU oracle's frame of that camera, as tests/test_gpu_configs.py compares, at the smallest shapes that reach each path:

  13x7 and 40x24            edge tiles with lanes outside the frame; one tile row and several
  1, 2 and 33 frames        each with its own camera: no division, the inline array, the device frame table
  RGBA16F and BGRA8         the 256- and the 512-entry table (one and two loads per lane, and the 513th entry)
  row-major, and TILES_RGBM14 shards of a two-shard partition (the tile list; that layout packs RGBA16F only)
  each launch twice         the centre-out order, then the learned one (the order entry's scalar load)
  both exact builds forced

and one case each of the supersampled, lens, ray-map, posed and shutter entry points at 13x7, which share the head,
against the references of their own tests (tests/test_gpu_forms_matrix.py, tests/test_gpu_rays_pose.py)."""
import functools

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
import oracle
from tests import _lens_ref, _rays_ref
from tests import _rays_pose_ref as pref
from tests import _scenarios as S
from tests import test_gpu_forms_matrix as forms
from tests import test_gpu_rays_pose as posed
from tests._cases import camera_uniform, uniforms
from tests._ss_ref import CAP, FLAGS, expected_bytes, sky_ss

pytestmark = pytest.mark.gpu

F32, F16, BGRA8 = bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB
DT = {F32: "float32", F16: "float16", BGRA8: "uint8"}
T = bh.BH_SCHED_TILE
BUILDS = [("issue-order build", T | bh.BH_SCHED_FLAG_ISSUE_ORDER), ("latency build", T | bh.BH_SCHED_FLAG_LATENCY)]
SIZES = [(13, 7), (40, 24)]
FRAMES = [1, 2, 33]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def scene(torch_cuda):
    s = bh.Scene(16, 16, sky=sky_ss(), max_iters=CAP, scene_flags=FLAGS, math=bh.BH_MATH_EXACT)
    s.uniforms = uniforms()
    yield s
    s.close()


def path_camera(i: int, W: int, H: int) -> bh.CameraUniform:
    """Frame i's camera: camera D (off-axis, close: disc, markers, shadow and sky in view) turned about the y axis
    through the hole by i x 9.7 degrees -- 33 frames, 33 cameras."""
    a = np.radians(9.7 * i)
    x, y, z = 7.0, 1.5, -9.0
    p = (float(x * np.cos(a) + z * np.sin(a)), y, float(-x * np.sin(a) + z * np.cos(a)))
    cu = bh.CameraUniform()
    cu.update(bh.Camera.look_at(p, (0.0, 0.0, 0.0), W, H))
    return cu


@functools.lru_cache(maxsize=None)
def oracle_frame(i: int, W: int, H: int):
    """(col, blackout_col) fp32 of frame i, once per process, read-only"""
    col, bo, _, _ = oracle.render_rows(path_camera(i, W, H).to_bytes(), bytes(uniforms().to_c()), sky_ss(), W, H, CAP, FLAGS)
    col.setflags(write=False)
    bo.setflags(write=False)
    return col, bo


def assert_bytes(got, want, what):
    got = got.cpu().numpy().view(np.uint8)
    bad = (got != np.ascontiguousarray(want).view(np.uint8).reshape(got.shape)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("fmt", [F16, BGRA8])
@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("W,H", SIZES)
def test_frames_rowmajor(torch_cuda, scene, W, H, n, fmt):
    torch = torch_cuda
    cams = [path_camera(i, W, H) for i in range(n)]
    dt = getattr(torch, DT[fmt])
    for build, schedule in BUILDS:
        for launch in ("centre-out order", "learned order"):
            cols = [torch.full((H, W, 4), 7, dtype=dt, device="cuda") for _ in cams]
            bos = [torch.full((H, W, 4), 7, dtype=dt, device="cuda") for _ in cams]
            scene.render_frames(cols, bos, cameras=cams, fmt=fmt, width=W, height=H, schedule=schedule)
            torch.cuda.synchronize()
            for i in range(n):
                oc, ob = oracle_frame(i, W, H)
                what = f"{W}x{H} n={n} fmt {fmt}, {build}, {launch}, frame {i}"
                assert_bytes(cols[i], expected_bytes(fmt, oc), what + ": col")
                assert_bytes(bos[i], expected_bytes(fmt, ob), what + ": blackout_col")


@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("W,H", SIZES)
def test_frames_partition_shards(torch_cuda, scene, W, H, n):
    """Two shards of a weighted partition in BH_LAYOUT_TILES_RGBM14 (col only: the blackout decision travels as the
    mask), unpacked to both targets."""
    torch = torch_cuda
    fmt, layout, SH = F16, bh.BH_LAYOUT_TILES_RGBM14, 2
    cams = [path_camera(i, W, H) for i in range(n)]
    part = bh.Partition(W, H, [1, 1])
    assert min(part.counts) > 0
    stride, tb = max(part.counts), bh.tile_bytes(layout, fmt)
    for build, schedule in BUILDS:
        for launch in ("centre-out order", "learned order"):
            packed = torch.zeros((SH * n * stride, tb), dtype=torch.uint8, device="cuda")
            for k in range(SH):
                blk = packed[k * n * stride:(k + 1) * n * stride]
                frames = [blk[f * stride:f * stride + part.counts[k]] for f in range(n)]
                scene.render_frames(frames, None, cameras=cams, fmt=fmt, width=W, height=H, schedule=schedule,
                                    layout=layout, shard_index=k, shard_count=SH, partition=part)
            for i in range(n):
                out_c = torch.full((H, W, 4), 7, dtype=torch.float16, device="cuda")
                out_b = torch.full_like(out_c, 7)
                bh.tiles_unpack_rgbm_partition(packed[i * stride:], out_c, out_b, part, n * stride, fmt | bh.BH_UNPACK_RGBM14)
                torch.cuda.synchronize()
                oc, ob = oracle_frame(i, W, H)
                what = f"{W}x{H} n={n} partition, {build}, {launch}, frame {i}"
                assert_bytes(out_c, expected_bytes(fmt, oc), what + ": col")
                assert_bytes(out_b, expected_bytes(fmt, ob), what + ": blackout_col")
    part.close()


# ---- the entry points that share the head, one case each at 13x7 ---------------------------------------------------
SCENARIO = S.BY_ID["disc_F2"]


def test_supersampled(torch_cuda):
    with forms.Scene(SCENARIO) as sc:
        forms.check_ss(torch_cuda, sc, SCENARIO, 13, 7, 2)


def test_lens(torch_cuda):
    want = _lens_ref.records(SCENARIO.camera, 13, 7, 1, SCENARIO.key)[0]
    with forms.Scene(SCENARIO) as sc:
        sc.camera_uniform = camera_uniform(SCENARIO.camera, 13, 7)
        for what, schedule in forms.PASSES:
            forms.assert_records(forms.lens_records(torch_cuda, sc, 13, 7, schedule), want, f"lens 13x7, {what}")


def test_ray_map(torch_cuda):
    s, W, H = SCENARIO, 13, 7
    with forms.Scene(s) as sc:
        forms.check_rays(torch_cuda, sc, s, _rays_ref.pinhole_map(s.camera, W, H), camera_uniform(s.camera, W, H).pos, W, H,
                         _lens_ref.frame(s.camera, W, H, "ctx", 1, s.key), "pinhole map",
                         dbg=_rays_ref.oracle_dbg(s.camera, W, H, s.key))


def test_shutter(torch_cuda):
    with forms.Scene(SCENARIO) as sc:
        forms.check_shutter(torch_cuda, sc, SCENARIO, 2, 13, 7)


def test_posed_ray_map_and_its_shutter(torch_cuda):
    torch, W, H = torch_cuda, 13, 7
    sc = posed.new_scene()
    sc.uniforms = uniforms()
    try:
        dirs = posed.upload(torch, pref.camera_map("general", W, H))
        for n in (2, 33):
            names = pref.sequence(n)
            for launch in range(2):
                posed.assert_frames(posed.render_frames(torch, sc, dirs, names, W, H), pref.frames(names, "general", W, H),
                                    F32, f"posed n {n}, launch {launch}")
        names = pref.sequence(2)
        for launch in range(2):
            posed.assert_frames(posed.render_shutter(torch, sc, dirs, [names], W, H), [pref.shutter(names, "general", W, H)],
                                F32, f"posed shutter, launch {launch}")
    finally:
        sc.close()
