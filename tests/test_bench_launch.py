"""bench.py's N-rank launcher and N>1 data path on CPU (gloo), without torchrun and without a GPU.

`python bench.py --gpus N` started without WORLD_SIZE must start its own N ranks before anything
touches a GPU, and must exit non-zero unless all N finish (VERDICT r01 "Next round" 1); the ranks of
the --plumbing mode run the same GatherPipeline and RGBM transport as the GPU path, with synthetic
shards packed by the host mirror of the march kernel's store and unpacked by the mirror of
bh_tiles_unpack_rgbm."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench(*args, env=None, timeout=240):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=e, cwd=str(ROOT))
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{"metric"')]
    return r.returncode, lines, r.stderr


@pytest.mark.parametrize("transport", ["rgbm14", "rgbm"])
@pytest.mark.parametrize("n", [2, 3])
def test_self_launch_runs_n_ranks_and_verifies_the_gather(n, transport):
    rc, lines, err = _bench("--gpus", str(n), "--plumbing", "--steps", "3", "--transport", transport)
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines            # rank 0 alone prints the line
    d = lines[0]
    assert d["n_gpus"] == n and d["world_size"] == n and d["backend"] == "gloo" and d["transport"] == transport
    assert d["frames_checked"] == 3 and d["gather_verified_bit_exact"] is True


def test_self_launch_fails_loudly_when_a_rank_fails():
    # rank 1 dies after joining the group (test hook); the launcher must stop rank 0, which would
    # otherwise wait in the gather, and return non-zero: never a line claiming n_gpus 2
    rc, lines, _ = _bench("--gpus", "2", "--plumbing", "--steps", "3", env={"BH_PLUMBING_FAIL_RANK": "1"})
    assert rc != 0
    assert all(d.get("gather_verified_bit_exact") is not True for d in lines)


def test_self_launch_deadline_stops_a_hung_rank():
    """A rank that hangs (not one that exits) must not hold the run for the driver's whole limit: the
    launcher's deadline stops every rank and prints one {"error": ...} line."""
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e["BH_PLUMBING_HANG_RANK"] = "1"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--plumbing", "--steps", "3",
                        "--deadline-s", "25", "--pg-timeout-s", "600"],
                       capture_output=True, text=True, timeout=120, env=e, cwd=str(ROOT))
    assert r.returncode != 0
    errs = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{"error"')]
    assert len(errs) == 1 and "deadline" in errs[0]["error"], r.stdout[-2000:]
    assert not any(x.startswith('{"metric"') for x in r.stdout.splitlines())


def test_process_group_timeout_ends_a_wedged_collective():
    """With the deadline out of the way, the process group's own timeout ends the wait of the rank
    blocked in the gather on the hung peer: it raises, exits non-zero, and the launcher stops the rest."""
    rc, lines, _ = _bench("--gpus", "2", "--plumbing", "--steps", "3", "--deadline-s", "600", "--pg-timeout-s", "8",
                          env={"BH_PLUMBING_HANG_RANK": "1"}, timeout=180)
    assert rc != 0
    assert all(d.get("gather_verified_bit_exact") is not True for d in lines)


def test_watchdog_ends_a_stalled_rank_well_inside_the_driver_limit():
    """A rank that stops making progress (here: the hang hook; on the node, a kernel or a collective that
    never returns) exits through its watchdog after --stall-s, and the launcher stops the rest and prints
    one {"error": ...} line -- long before the deadline and the driver's 600 s."""
    import time
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e["BH_PLUMBING_HANG_RANK"] = "1"
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--plumbing", "--steps", "3",
                        "--stall-s", "4", "--deadline-s", "300", "--pg-timeout-s", "300"],
                       capture_output=True, text=True, timeout=200, env=e, cwd=str(ROOT))
    took = time.monotonic() - t0
    assert r.returncode != 0
    assert took < 100, took
    errs = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{"error"')]
    assert len(errs) == 1 and "watchdog" in errs[0]["error"], r.stdout[-2000:] + r.stderr[-2000:]
    assert "no progress" in r.stderr
    assert not any(x.startswith('{"metric"') for x in r.stdout.splitlines())


def test_default_deadline_is_below_the_driver_limit():
    sys.path.insert(0, str(ROOT))
    import bench
    a = bench.parse([])
    assert 0 < a.deadline_s <= 450 and 0 < a.stall_s < a.deadline_s


def test_frames_per_launch_is_capped_by_rank0_bytes():
    """N > 1: 64 frames per batch, fewer when rank 0's targets and receive slots of a batch would pass the
    byte budget (16384 x 8192 frames at 64 would not fit)."""
    sys.path.insert(0, str(ROOT))
    import bench
    assert bench.auto_frames_per_launch(8, 8192, 4096, 512) == 64
    D = bench.auto_frames_per_launch(8, 16384, 8192, 512)
    assert 1 <= D < 64
    per_frame = 2 * 16384 * 8192 * 8 + 2 * (16384 // 8) * (8192 // 8) * 344
    assert D * per_frame <= bench.RANK0_FRAME_BYTES


def test_world_size_mismatch_is_refused():
    rc, lines, err = _bench("--gpus", "2", "--plumbing", env={"WORLD_SIZE": "3", "RANK": "0"})
    assert rc != 0 and not lines
    assert "refusing" in err


@pytest.mark.parametrize("cfg,want", [(1, (256, 256, 64, "A", "off", "strong")), (2, (1920, 1080, 256, "B", "on", "strong")),
                                      (3, (0, 0, 512, "A", "on", "strong")), (4, (0, 0, 512, "A", "on", "config4")),
                                      (5, (0, 0, 1000, "C", "on", "strong"))])
def test_config_flag_maps_the_baseline_configs(cfg, want):
    """bench.py --config N selects BASELINE.json configs[N-1] (frame, cap, camera, scene, workload)."""
    sys.path.insert(0, str(ROOT))
    import bench
    a = bench.apply_config(bench.parse(["--config", str(cfg)]))
    assert (a.width, a.height, a.max_iters, a.camera, a.surfaces, a.workload) == want


def test_rccl_dry_run_needs_one_rank():
    rc, lines, err = _bench("--gpus", "2", "--rccl-dry-run", env={"WORLD_SIZE": "2"})
    assert rc != 0 and not lines and "one rank" in err


@pytest.mark.gpu
def test_rccl_dry_run_gathers_bit_exact():
    """The N>1 code path at one rank over a real RCCL group (nccl backend): RGBM shard render,
    pipelined dist.gather on the GPU, rank-0 unpack of both targets, barrier and the max-over-ranks
    all_gather -- the collectives the driver's 8-GPU run makes, checked on a 1-GPU box."""
    pytest.importorskip("torch")
    rc, lines, err = _bench("--gpus", "1", "--rccl-dry-run", "--verify-gather", "--steps", "16", "--warmup", "8",
                            "--width", "1024", "--height", "512", timeout=300)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    d = lines[0]
    assert d["backend"] == "nccl" and d["world_size"] == 1 and d["n_gpus"] == 1
    assert d["gather_verified_bit_exact"] is True
    assert "RCCL DRY RUN" in d["config"]["parallelism"]


def test_steps_are_batches_and_the_settle_is_optional():
    """A step is one batch (one bh_render_frames launch of D frames, VERDICT/ADVICE r02): the driver's
    --steps / --warmup count batches and are never changed; the power-state settle of round 2 is off
    by default (the warm-up batches cover the clock ramp) and can still be asked for."""
    sys.path.insert(0, str(ROOT))
    import bench
    a = bench.parse(["--warmup", "5", "--steps", "20"])
    assert a.settle_ms == 0.0 and a.warmup == 5 and a.steps == 20
    assert bench.parse(["--settle-ms", "100"]).settle_ms == 100.0
    assert bench.auto_frames_per_launch(1, 4096, 2048, 512) == 32
    assert bench.auto_frames_per_launch(8, 4096, 2048, 512) == 64


def test_a_plain_run_is_the_default_and_full_is_an_option():
    sys.path.insert(0, str(ROOT))
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs == "" and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.parametrize("W,H,D,dtype", [(24, 10, 3, "float16"), (4096, 2048, 32, "float16"), (40, 16, 2, "uint8")])
def test_dump_outputs_writes_float32_samples_within_the_budget(tmp_path, W, H, D, dtype):
    """--dump-outputs: every pixel of a small frame, a fixed sorted sample of a large one; float32 copies of
    the targets' words at those pixels; the same files from call to call."""
    torch = pytest.importorskip("torch")
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import bench
    base = torch.arange(H * W * 4, dtype=torch.int32).reshape(H, W, 4) % 251
    cols = [(base + f).to(getattr(torch, dtype)) for f in range(2)] * (D // 2) + [base.to(getattr(torch, dtype))] * (D % 2)
    bos = [c // 2 for c in cols] if dtype == "uint8" else [c * 0.5 for c in cols]
    bench.dump_outputs(tmp_path / "a", cols, bos, W, H, torch)
    bench.dump_outputs(tmp_path / "b", cols, bos, W, H, torch)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["blackout_col.npy", "col.npy", "pixel_index.npy"]
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= 64_000_000
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    col, bo = np.load(tmp_path / "a" / "col.npy"), np.load(tmp_path / "a" / "blackout_col.npy")
    assert idx.dtype == np.float64 and col.dtype == np.float32 and bo.dtype == np.float32
    P = W * H if W * H * D * 32 <= bench.DUMP_BYTES else bench.DUMP_BYTES // (32 * D)
    assert col.shape == bo.shape == (D, P, 4) and idx.shape == (P,)
    i = idx.astype(np.int64)
    assert np.all(np.diff(i) > 0) and i[0] >= 0 and i[-1] < W * H
    for f in (0, D - 1):
        assert np.array_equal(col[f], cols[f].reshape(-1, 4).numpy()[i].astype(np.float32))
        assert np.array_equal(bo[f], bos[f].reshape(-1, 4).numpy()[i].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_frames(tmp_path):
    """A plain run (no --full) on the GPU: the line keeps the headline keys, carries none of the legs that
    take runs of their own, --steps is the number of timed launches, and the dumped frames are the
    scene's exact-math render bit for bit (every frame of a fixed-camera batch is that frame)."""
    torch = pytest.importorskip("torch")
    import numpy as np
    import black_hole_ray_marching_amd as bh
    W, H, cap = 104, 56, 64
    rc, lines, err = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--width", str(W), "--height", str(H),
                            "--max-iters", str(cap), "--frames-per-launch", "2", "--dump-outputs", str(tmp_path / "o"))
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    d = lines[0]
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["value"] > 0
    assert d["steps"] == 3 and d["kernel"]["launches"] == 3 and d["ms_per_step"] > 0
    assert abs(d["value"] - W * H * 2 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["kernel"]["sum_steps"] is None
    assert "single_frame" not in d and "orbit" not in d and "parity" not in d
    scene = bh.Scene(W, H, sky=bh.synthetic_sky(4096, 2048), device=0, max_iters=cap, math=bh.BH_MATH_EXACT)
    col = torch.empty((H, W, 4), dtype=torch.float16, device="cuda:0")
    bo = torch.empty_like(col)
    scene.render(col, bo, fmt=bh.BH_OUT_RGBA16F)
    torch.cuda.synchronize()
    scene.close()
    got_c, got_b = np.load(tmp_path / "o" / "col.npy"), np.load(tmp_path / "o" / "blackout_col.npy")
    assert got_c.shape == (2, W * H, 4) and got_c.dtype == np.float32
    for f in range(2):
        assert np.array_equal(got_c[f], col.cpu().numpy().reshape(-1, 4).astype(np.float32))
        assert np.array_equal(got_b[f], bo.cpu().numpy().reshape(-1, 4).astype(np.float32))


@pytest.mark.gpu
def test_full_run_carries_the_legs_beside_the_headline():
    """--full: the step-count launch (roofline, kernel.sum_*), the single_frame / orbit legs and the CPU leg
    (cpu_baseline, parity against the oracle, bit-exact in exact math) follow the timed steps."""
    pytest.importorskip("torch")
    W, H = 104, 72  # the CPU leg warms the oracle up on rows 0..63
    rc, lines, err = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--width", str(W), "--height", str(H),
                            "--max-iters", "64", "--frames-per-launch", "2", "--cpu-reps", "1", "--full")
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    d = lines[0]
    assert d["steps"] == 3 and d["kernel"]["launches"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert 0 < d["kernel"]["sum_steps"] <= d["kernel"]["sum_n_rk"] <= 64 * W * H
    assert d["roofline"]["bound"] == "valu" and 0 < d["roofline"]["frac"] < 1
    for leg in ("single_frame", "orbit", "single_frame_orbit"):
        assert d[leg]["ms_per_frame"] > 0
    assert d["cpu_baseline"]["value"] > 0
    assert d["parity"]["pixels"] == W * H and d["parity"]["bit_exact"] is True
    assert d["parity"]["timed_format_bit_exact"] is True


def test_clock_accumulators_to_mhz():
    """bh_set_clock_probe's per-XCD accumulators (shader ticks, 100 MHz ticks, waves) -> MHz."""
    import numpy as np
    import black_hole_ray_marching_amd as bh
    acc = np.zeros(128, np.int64)
    acc[0:3] = (2_100_000, 100_000, 10)       # XCD 0: 2100 MHz
    acc[16:19] = (2_300_000, 100_000, 10)     # XCD 1: 2300 MHz
    c = bh.clock_mhz(acc)
    assert c["mhz"] == 2200.0 and c["per_xcd_mhz"][:2] == [2100.0, 2300.0] and c["per_xcd_mhz"][2] is None
    assert c["waves"] == 20 and c["wave_ms"] == 0.1  # 1 ms of 100 MHz ticks per 10 waves
