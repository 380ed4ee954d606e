"""GPU parity at the input edges the reference's key bindings reach (tests/_cases.py EDGE_CASES): the domain
guards of the correctly rounded cores (bh_crmath.hpp, bh_march_step.hpp step_bf) and the host's specialisation
gates (bh_host.cpp fill_args, sdf_far_r2), with whole frames.

tests/test_edge_inputs.py shows on the CPU that the oracle is well defined on every case and that each case
reaches the guard it aims at (tests/_domain_census.py); here the kernels must give the oracle's bits.
  * BH_MATH_EXACT: every output word, n_rk and fate equal to oracle/bh_oracle.c, under every schedule and
    both dispatch orders, in every output format, and with frames of different cameras in one launch;
  * BH_MATH_FAST promises no bits: only that every output is a valid one."""
import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from tests._cases import EDGE, EDGE_CASES, EDGE_IDS, camera_uniform, uniforms
from tests._gpu_common import SCHEDULES, assert_bitexact, bgra8_expected, gpu_render, oracle_render

pytestmark = pytest.mark.gpu

EDGE_SCHEDULES = SCHEDULES + [bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_STATIC_ORDER]
SCHED_IDS = ["pair", "tile_issue", "tile_latency", "persistent", "tile_static"]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def scene_small(torch_cuda, sky_small):
    scene = bh.Scene(16, 16, sky=sky_small)
    yield scene
    scene.close()


@pytest.fixture(scope="module")
def edge_oracle(sky_small):
    """The oracle's frame of an edge case, computed once per case and shared (never written to)."""
    cache = {}

    def get(case_id):
        if case_id not in cache:
            cam, W, H, cap, flags, over = EDGE[case_id]
            o = oracle_render(camera_uniform(cam, W, H), uniforms(**over), sky_small, W, H, cap, flags)
            for a in o:
                a.setflags(write=False)
            cache[case_id] = o
        return cache[case_id]
    return get


def _is_tile(schedule):
    return (schedule & 0xFF) == bh.BH_SCHED_TILE


@pytest.mark.parametrize("schedule", EDGE_SCHEDULES, ids=SCHED_IDS)
@pytest.mark.parametrize("case_id", EDGE_IDS)
def test_exact_bitexact_at_the_edges(torch_cuda, scene_small, edge_oracle, case_id, schedule):
    """Bit-exact against the oracle, twice: the second render of the tile schedule runs in the dispatch
    order learned from the first.  dbg_steps (iterations executed) never exceeds dbg_n_rk."""
    cam, W, H, cap, flags, over = EDGE[case_id]
    cu, U = camera_uniform(cam, W, H), uniforms(**over)
    o = edge_oracle(case_id)
    for rep in range(2):
        g = gpu_render(torch_cuda, scene_small, cu, U, W, H, cap, flags, bh.BH_MATH_EXACT, schedule=schedule,
                       steps=True)
        assert_bitexact(g[:4], o)
        nrk, steps = g[2], g[4]
        assert (steps <= nrk).all(), f"render {rep}: dbg_steps > dbg_n_rk at {np.argwhere(steps > nrk)[:5]}"
        if case_id == "dtm_zero":
            # every ray sits still: a period-1 exact cycle from the first step, so the tile schedule's
            # cycle fast-forward takes each ray to the cap without iterating
            assert (nrk == cap).all() and (g[3] == bh.BH_FATE_CAP).all()
            if _is_tile(schedule):
                assert (steps < nrk).any()


FORMAT_CASES = ["big_s_f3", "near5_f3", "origin_bo0"]


@pytest.mark.parametrize("case_id", FORMAT_CASES)
def test_fp16_output_is_rne_of_exact_at_the_edges(torch_cuda, scene_small, edge_oracle, case_id):
    cam, W, H, cap, flags, over = EDGE[case_id]
    cu, U = camera_uniform(cam, W, H), uniforms(**over)
    g16 = gpu_render(torch_cuda, scene_small, cu, U, W, H, cap, flags, bh.BH_MATH_EXACT, fmt=bh.BH_OUT_RGBA16F,
                     schedule=bh.BH_SCHED_TILE)
    oc, ob, on, of = edge_oracle(case_id)
    assert np.array_equal(g16[0].view(np.uint16), oc.astype(np.float16).view(np.uint16))
    assert np.array_equal(g16[1].view(np.uint16), ob.astype(np.float16).view(np.uint16))
    assert np.array_equal(g16[2], on) and np.array_equal(g16[3], of)


@pytest.mark.parametrize("case_id", FORMAT_CASES)
def test_bgra8_srgb_output_is_encoded_exact_result_at_the_edges(torch_cuda, scene_small, edge_oracle, case_id):
    torch = torch_cuda
    cam, W, H, cap, flags, over = EDGE[case_id]
    scene_small.camera_uniform, scene_small.uniforms = camera_uniform(cam, W, H), uniforms(**over)
    scene_small.max_iters, scene_small.scene_flags = cap, flags
    col = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    bo = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    scene_small.render(col, bo, fmt=bh.BH_OUT_BGRA8_SRGB, math=bh.BH_MATH_EXACT, width=W, height=H,
                       schedule=bh.BH_SCHED_TILE)
    torch.cuda.synchronize()
    o = edge_oracle(case_id)
    assert np.array_equal(col.cpu().numpy(), bgra8_expected(o[0]))
    assert np.array_equal(bo.cpu().numpy(), bgra8_expected(o[1]))


def test_frames_of_far_near_default_and_origin_cameras_in_one_launch(torch_cuda, sky_small):
    """One render_frames launch of 4 frames under one uniform set: a far camera (Q > 2^60), a near one
    (Q < 2^-40), camera A and the origin camera (NaN state).  The SF_CAM_OUT choice is per wave and the
    frames interleave in one grid: each frame equals its single render and the oracle."""
    torch = torch_cuda
    W, H, cap, flags = 44, 28, 128, 3
    cams = ["FAR", "NEAR3", "A", "ORIGIN"]
    U = uniforms(blackout_eh=0, max_dist=20000.0)
    cus = [camera_uniform(c, W, H) for c in cams]
    scene = bh.Scene(W, H, sky=sky_small, max_iters=cap, scene_flags=flags, math=bh.BH_MATH_EXACT)
    scene.uniforms = U
    n = len(cams)
    cols = [torch.full((H, W, 4), float("nan"), device="cuda") for _ in range(n)]
    bos = [torch.full((H, W, 4), float("nan"), device="cuda") for _ in range(n)]
    nrks = [torch.full((H, W), -1, dtype=torch.int16, device="cuda") for _ in range(n)]
    fates = [torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(n)]
    steps = [torch.full((H, W), -1, dtype=torch.int16, device="cuda") for _ in range(n)]
    scene.render_frames(cols, bos, cameras=cus, dbg_n_rk=nrks, dbg_fate=fates, dbg_steps=steps,
                        schedule=bh.BH_SCHED_TILE)
    torch.cuda.synchronize()
    for i, cam in enumerate(cams):
        g = (cols[i].cpu().numpy(), bos[i].cpu().numpy(), nrks[i].cpu().numpy().view(np.uint16),
             fates[i].cpu().numpy())
        st = steps[i].cpu().numpy().view(np.uint16)
        single = gpu_render(torch, scene, cus[i], U, W, H, cap, flags, bh.BH_MATH_EXACT, schedule=bh.BH_SCHED_TILE,
                            steps=True)
        o = oracle_render(cus[i], U, sky_small, W, H, cap, flags)
        assert_bitexact(g, o)
        assert_bitexact(g, single[:4])
        assert (st <= g[2]).all(), cam
    scene.close()


@pytest.mark.parametrize("cam,W,H,cap,flags,over", EDGE_CASES, ids=EDGE_IDS)
def test_fast_mode_outputs_are_valid_at_the_edges(torch_cuda, scene_small, cam, W, H, cap, flags, over):
    """BH_MATH_FAST promises no bits on these inputs, only valid outputs, under the tile, pair and persistent
    schedules (three kernels, two forms of the step): a fate in 0..3, n_rk <= cap, every
    colour channel finite and in [0, 1], alpha 1, and the blackout target the per-pixel function of col
    (src/black_hole_maybe.wgsl:365-368).  No comparison with the oracle's colours."""
    cu, U = camera_uniform(cam, W, H), uniforms(**over)
    for schedule in (bh.BH_SCHED_TILE, bh.BH_SCHED_PAIR, bh.BH_SCHED_PERSISTENT):
        gc, gb, gn, gf = gpu_render(torch_cuda, scene_small, cu, U, W, H, cap, flags, bh.BH_MATH_FAST,
                                    schedule=schedule)
        assert gf.max() <= 3, (schedule, np.unique(gf))
        assert int(gn.max()) <= cap, schedule
        assert np.isfinite(gc).all(), f"schedule {schedule}: non-finite colour at {np.argwhere(~np.isfinite(gc))[:5]}"
        assert (gc[..., :3] >= 0).all() and (gc[..., :3] <= 1).all() and (gc[..., 3] == 1).all(), schedule
        keep = ~(((gc[..., 0] * gc[..., 0] + gc[..., 1] * gc[..., 1]) + gc[..., 2] * gc[..., 2]) < 1.0)
        exp = np.where(keep[..., None], gc, np.array([0, 0, 0, 1], np.float32))
        assert np.array_equal(gb, exp), schedule
