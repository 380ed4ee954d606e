"""Iteration 0 from the frame's first-step record (csrc/bh_march_step.hpp, step_first), on the GPU: every case against
the CPU oracle bit for bit -- both targets, dbg_n_rk and dbg_fate where the form has them.  The oracle has no count of
executed steps, so dbg_steps is held to what the oracle does fix: it equals n_rk on every ray that is not capped, and
never exceeds it on a capped one (the cycle fast-forward, which now begins its search one iteration later).
Each case first asserts, from bh_first_step_host, that its frame's record is valid (or not), so that none passes by
being off; tests/test_first_step_host.py ties that function to the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd.scene import first_step_host
from tests import _lens_ref, _rays_pose_ref, _rays_ref
from tests import _scenarios as S
from tests import test_gpu_forms_matrix as M
from tests._cases import camera_uniform, uniforms
from tests._gpu_common import assert_bitexact, gpu_render, oracle_render
from tests._ss_ref import scenario_uniforms, sky_ss

pytestmark = pytest.mark.gpu

F32, F16, BGRA8 = M.F32, M.F16, M.BGRA8
T = bh.BH_SCHED_TILE
BUILDS = [("issue-order build", T | bh.BH_SCHED_FLAG_ISSUE_ORDER), ("latency build", T | bh.BH_SCHED_FLAG_LATENCY)]
SIZES = [(8, 8), (13, 7), (24, 16)]   # one tile; partial tiles on both axes; six whole tiles


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def scene(torch_cuda):
    sc = bh.Scene(16, 16, sky=sky_ss(), math=bh.BH_MATH_EXACT)
    yield sc
    sc.close()


def look(pos, target=(0.0, 0.0, 0.0), W=16, H=16) -> bh.CameraUniform:
    cu = bh.CameraUniform()
    cu.update(bh.Camera.look_at(pos, target, W, H))
    return cu


def check_plain(torch, sc, cu, U, W, H, cap, flags, valid, what):
    """One frame in both exact builds against the oracle; `valid`: what its record must be."""
    assert first_step_host(cu, U, flags, cap)[0] == valid, f"{what}: the record's validity"
    want = oracle_render(cu, U, sky_ss(), W, H, cap, flags)
    for name, schedule in BUILDS:
        *got, steps = gpu_render(torch, sc, cu, U, W, H, cap, flags, bh.BH_MATH_EXACT, schedule=schedule, steps=True)
        assert_bitexact(tuple(got), want)
        n_rk, fate = got[2], got[3]
        free = fate != bh.BH_FATE_CAP
        assert np.array_equal(steps[free], n_rk[free]) and (steps <= n_rk).all(), f"{what}, {name}: dbg_steps"


# (id, camera, uniform overrides, cap, flags, the record is valid)
CAMERA_CASES = [
    ("A", lambda W, H: camera_uniform("A", W, H), {}, 64, 3, True),
    ("B", lambda W, H: camera_uniform("B", W, H), {}, 64, 3, True),
    ("C", lambda W, H: camera_uniform("C", W, H), {}, 64, 3, True),   # dt0 from a marker, not dtm r
    ("inside_r0p3", lambda W, H: camera_uniform("IN03", W, H), {}, 64, 3, False),
    ("marker_surface", lambda W, H: look((0.0, 10.0, -10.5), W=W, H=H), {}, 64, 3, False),
    ("max_dist_below_dt0", lambda W, H: camera_uniform("A", W, H), {"max_dist": 5.0}, 64, 3, False),
    ("max_iters_1", lambda W, H: camera_uniform("A", W, H), {}, 1, 3, False),
    ("dtm_zero", lambda W, H: camera_uniform("B", W, H), {"delta_time_mult": 0.0}, 64, 3, False),
    ("rs_nan", lambda W, H: camera_uniform("B", W, H), {"rs": float("nan")}, 16, 3, False),
]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("case", CAMERA_CASES, ids=[c[0] for c in CAMERA_CASES])
def test_cameras(torch_cuda, scene, case, W, H):
    name, cam, over, cap, flags, valid = case
    check_plain(torch_cuda, scene, cam(W, H), uniforms(**over), W, H, cap, flags, valid, f"{name} {W}x{H}")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("sid", S.IDS)
def test_scenarios_plain(torch_cuda, scene, sid, W, H):
    """The scenario table in the plain form; its long caps run the cycle fast-forward from one iteration later."""
    s = S.BY_ID[sid]
    cu, U = camera_uniform(s.camera, W, H), scenario_uniforms(s.key)
    check_plain(torch_cuda, scene, cu, U, W, H, s.cap, s.flags, first_step_host(cu, U, s.flags, s.cap)[0], f"{sid} {W}x{H}")


def test_scenarios_cover_both_sides_of_the_gate():
    valid = {s.id: first_step_host(camera_uniform(s.camera, 13, 7), scenario_uniforms(s.key), s.flags, s.cap)[0] for s in S.TABLE}
    assert valid["long_odd"] and valid["none_E"] and valid["disc_D"] and not valid["none_F2"] and not valid["big_s_f3"], valid


@pytest.mark.parametrize("cap", [1, 2, 3, 48, 49, 50, 192, 193])
def test_caps(torch_cuda, scene, cap):
    """The cap test at iteration 1 (cap 2), the hand-over to the tail's loop (48 before, 49 now) and the end of the
    cycle search (192), on camera E's capped rays."""
    check_plain(torch_cuda, scene, camera_uniform("E", 24, 16), uniforms(), 24, 16, cap, 3, cap >= 2, f"E cap {cap}")


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_scene_flags(torch_cuda, scene, flags):
    check_plain(torch_cuda, scene, camera_uniform("C", 13, 7), uniforms(), 13, 7, 64, flags, True, f"C flags {flags}")


@pytest.mark.parametrize("fmt", [F32, F16, BGRA8])
def test_formats(torch_cuda, scene, fmt):
    torch, (W, H) = torch_cuda, (13, 7)
    cu, U = camera_uniform("C", W, H), uniforms()
    assert first_step_host(cu, U, 3, 64)[0]
    oc, ob, _, _ = oracle_render(cu, U, sky_ss(), W, H, 64, 3)
    scene.camera_uniform, scene.uniforms, scene.max_iters, scene.scene_flags = cu, U, 64, 3
    for name, schedule in BUILDS:
        col, bo = M.pixels(torch, W, H, fmt), M.pixels(torch, W, H, fmt)
        scene.render(col.ptr, bo.ptr, fmt=fmt, math=bh.BH_MATH_EXACT, width=W, height=H, schedule=schedule)
        torch.cuda.synchronize()
        M.assert_pair(col, bo, (oc, ob), fmt, f"C fmt {fmt}, {name}")


@pytest.mark.parametrize("n", [2, 33])
def test_frames_each_with_its_own_record(torch_cuda, scene, n):
    """2 frames ride in the kernel argument, 33 behind the staged table; every frame has a camera of its own and one
    of them (the second) has no record: validity is per frame."""
    torch, (W, H), cap = torch_cuda, (13, 7), 64
    cams = [look((0.3 * i, 2.0 + 0.25 * i, -18.0 + 0.4 * i), W=W, H=H) for i in range(n)]
    cams[1] = camera_uniform("IN03", W, H)
    U = uniforms()
    valid = [first_step_host(c, U, 3, cap)[0] for c in cams]
    assert valid == [i != 1 for i in range(n)]
    scene.uniforms, scene.max_iters, scene.scene_flags = U, cap, 3
    want = [oracle_render(c, U, sky_ss(), W, H, cap, 3) for c in cams]
    for name, schedule in BUILDS:
        cols = [torch.full((H, W, 4), float("nan"), device="cuda") for _ in cams]
        bos = [torch.full((H, W, 4), float("nan"), device="cuda") for _ in cams]
        nrks = [torch.full((H, W), -1, dtype=torch.int16, device="cuda") for _ in cams]
        fates = [torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda") for _ in cams]
        scene.render_frames(cols, bos, cameras=cams, dbg_n_rk=nrks, dbg_fate=fates, math=bh.BH_MATH_EXACT, width=W, height=H,
                            schedule=schedule)
        torch.cuda.synchronize()
        for i in range(n):
            assert_bitexact((cols[i].cpu().numpy(), bos[i].cpu().numpy(), nrks[i].cpu().numpy().view(np.uint16),
                             fates[i].cpu().numpy()), want[i])


FS_C = S.Scenario("first_step_C", "C", 64, 3, (), "camera C: a valid record whose dt0 is not dtm r")
BUILD_PASSES = [(name, schedule) for name, schedule in BUILDS]


def test_derived_forms_on_camera_c(torch_cuda):
    """One case each of ss = 2, shutter n = 2, lens, ray map and posed ray map with camera C's record, in both builds."""
    torch, s, (W, H) = torch_cuda, FS_C, (13, 7)
    cu = camera_uniform("C", W, H)
    assert first_step_host(cu, uniforms(), 3, 64)[0]
    with M.Scene(s) as sc:
        M.check_ss(torch, sc, s, W, H, 2, passes=BUILD_PASSES)
        M.check_shutter(torch, sc, s, 2, W, H, passes=BUILD_PASSES)
        sc.camera_uniform = cu
        want = _lens_ref.records("C", W, H, 1, s.key)[0]
        for name, schedule in BUILDS:
            M.assert_records(M.lens_records(torch, sc, W, H, schedule), want, f"C lens, {name}")
        M.check_rays(torch, sc, s, _rays_ref.pinhole_map("C", W, H), cu.pos, W, H, _lens_ref.frame("C", W, H, "ctx", 1, s.key),
                     "pinhole map", dbg=_rays_ref.oracle_dbg("C", W, H, s.key), passes=BUILD_PASSES)
        # a camera-space equirect map turned by a rotated basis at C's position
        pose = np.concatenate([cu.pos[None, :], _rays_pose_ref.NAMED["rotH"][1]]).astype(np.float32)
        m = _rays_ref.equirect_map(W, H)
        wc, wb, _, _, _ = _rays_ref.trace(_rays_pose_ref.apply_np(pose, m), pose[0], s.key)
        d = M.upload(torch, m)
        for name, schedule in BUILDS:
            col, bo = M.pixels(torch, W, H), M.pixels(torch, W, H)
            sc.render_frames_rays(d, [col.ptr], [bo.ptr], poses=[pose], width=W, height=H, schedule=schedule)
            torch.cuda.synchronize()
            M.assert_pair(col, bo, (wc, wb), F32, f"C posed map, {name}")


def test_origin_map_is_unchanged(torch_cuda):
    """The origin-map form takes no record (its rays start at the lane's origin): its traces as before."""
    s = S.BY_ID["far_off"]
    with M.Scene(s) as sc:
        M.check_posed(torch_cuda, sc, s, F32, 1, True)


_CHILD = """
import sys
import numpy as np, torch
import black_hole_ray_marching_amd as bh
from tests._cases import camera_uniform, uniforms
from tests._gpu_common import gpu_render
from tests._ss_ref import sky_ss
sc = bh.Scene(16, 16, sky=sky_ss(), math=bh.BH_MATH_EXACT)
out = {}
for cam in ("A", "C", "E"):
    g = gpu_render(torch, sc, camera_uniform(cam, 24, 16), uniforms(), 24, 16, 64, 3, bh.BH_MATH_EXACT,
                   schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_ISSUE_ORDER)
    out.update({f"{cam}{i}": a for i, a in enumerate(g)})
sc.close()
np.savez(sys.argv[1], **out)
"""


def test_switch_gives_the_same_bytes(torch_cuda, tmp_path):
    """A child process with BH_NO_FIRST_STEP set (no frame has a record) renders the oracle's bytes too."""
    env = dict(os.environ, BH_NO_FIRST_STEP="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "frames.npz")
    out = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.load(path)
    for cam in ("A", "C", "E"):
        want = oracle_render(camera_uniform(cam, 24, 16), uniforms(), sky_ss(), 24, 16, 64, 3)
        assert_bitexact(tuple(got[f"{cam}{i}"] for i in range(4)), want)
