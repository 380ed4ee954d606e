"""Filtered lens shades on the GPU (bh_sky_create_mips / bh_shade_lens_mip; bh.Sky(mips=True), Scene.shade(mip=True)):
the chain's levels and every shade equal tests/_lens_mip_ref.py's numpy restatement of include/bh_render.h, bit
for bit.  The reference is never the GPU's output and never the library's host mirror; lenses are the CPU oracle's
records (tests/_lens_ref.py) or hand-made, uploaded from the host, and in the end-to-end test the GPU's own
render_lens (whose records tests/test_gpu_lens.py holds to the same oracle records)."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._cases import camera_uniform, uniforms
from tests._lens_mip_ref import SKIES, hand_grids, level_np, mips_np, n_levels_of, shade_mip_np, shade_mip_ref, sky
from tests._lens_ref import CAMS, SIZES, frame, records
from tests._ss_ref import CAP, FLAGS, expected_bytes, sky_ss

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}
F32 = bh.BH_OUT_RGBA32F
SENTINEL = 0xA5  # every byte of a buffer before a call
GUARD = 256      # bytes before and after a target that must keep their sentinels
SS_VIEWS = [(13, 7, 2), (13, 7, 4), (40, 24, 2)]


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
    s.mip_skies = {n: bh.Sky(s, sky(n), mips=True) for n in SKIES}
    yield s
    s.close()


class Target:
    """A W x H target of `fmt` between two guard regions, every byte the sentinel"""

    def __init__(self, torch, W, H, fmt):
        n = W * H * _abi.BYTES_PER_PIXEL[fmt]
        self.whole = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.whole[GUARD:GUARD + n].view(getattr(torch, DT[fmt])).view(H, W, 4)
        self.n = n

    def bytes(self):
        """the target's bytes, after checking both guards"""
        b = self.whole.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all(), "the guard region before the target was written"
        assert (b[GUARD + self.n:] == SENTINEL).all(), "the guard region after the target was written"
        return b[GUARD:GUARD + self.n].reshape(self.t.shape[0], self.t.shape[1], -1)

    def untouched(self):
        return bool((self.whole.cpu().numpy() == SENTINEL).all())


def assert_frame(got, want, what, where=None):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(got.shape)
    bad = (got != want).any(-1)
    if where is not None:
        bad &= where
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def upload(torch, rec):
    return torch.from_numpy(np.array(rec, np.float32)).cuda()


def shade(torch, sc, lens, W, H, sky_name, fmt=F32, blackout=True, ss=1, mip=True, **kw):
    """(col bytes, blackout bytes or None) of Scene.shade(mip=True) into guarded sentinel-filled targets"""
    col = Target(torch, W, H, fmt)
    bo = Target(torch, W, H, fmt) if blackout else None
    sc.shade(lens, col.t, None if bo is None else bo.t, fmt=fmt, sky=sc.mip_skies[sky_name], ss=ss, width=W, height=H, mip=mip, **kw)
    torch.cuda.synchronize()
    return col.bytes(), None if bo is None else bo.bytes()


@pytest.mark.parametrize("sky_name", SKIES)
def test_levels_equal_the_reference(torch_cuda, scene, sky_name):
    k = scene.mip_skies[sky_name]
    chain = mips_np(sky_name)
    assert k.levels == len(chain) == n_levels_of(k.width, k.height)
    for l in range(1, len(chain)):
        got = k.level(l)
        assert got.shape == chain[l].shape and np.array_equal(got.view(np.uint16), chain[l].view(np.uint16)), f"level {l}"
    plain = bh.Sky(scene, sky(sky_name))
    try:
        assert plain.levels == 0
        for l in (0, 1):
            with pytest.raises(bh.BhError) as e:
                plain.level(l)
            assert e.value.status == _abi.BH_ERR_INVALID_ARG
    finally:
        plain.close()
    for l in (0, len(chain)):
        with pytest.raises(bh.BhError) as e:
            k.level(l)
        assert e.value.status == _abi.BH_ERR_INVALID_ARG


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("cam", CAMS)
def test_shade_of_oracle_records(torch_cuda, scene, cam, W, H):
    lens = upload(torch_cuda, records(cam, W, H)[0])
    for sky_name in SKIES:
        wc, wb = shade_mip_ref(cam, W, H, sky_name)
        col, bo = shade(torch_cuda, scene, lens, W, H, sky_name)
        assert_frame(col, wc, f"{sky_name} col")
        assert_frame(bo, wb, f"{sky_name} blackout_col")


@pytest.mark.parametrize("W,H,k", SS_VIEWS)
@pytest.mark.parametrize("cam", ["E", "H"])
def test_shade_of_oracle_records_ss(torch_cuda, scene, cam, W, H, k):
    lens = upload(torch_cuda, records(cam, W, H, k)[0])
    for sky_name in SKIES:
        wc, wb = shade_mip_ref(cam, W, H, sky_name, k)
        col, bo = shade(torch_cuda, scene, lens, W, H, sky_name, ss=k)
        assert_frame(col, wc, f"{sky_name} ss={k} col")
        assert_frame(bo, wb, f"{sky_name} ss={k} blackout_col")


@pytest.mark.parametrize("sky_name", SKIES)
def test_shade_of_hand_made_grids(torch_cuda, scene, sky_name):
    """70 x 9 pixels: both neighbour directions cross wave and workgroup borders; 1-wide and 1-high grids; the
    last-level clamp, the exact powers of two, the seam, NaNs and sentinels as centres and as neighbours."""
    for name, (g, k) in hand_grids().items():
        H, W = g.shape[0] // k, g.shape[1] // k
        wc, wb = shade_mip_np(g, sky_name, k)
        col, bo = shade(torch_cuda, scene, upload(torch_cuda, g), W, H, sky_name, ss=k)
        assert_frame(col, wc, f"{name} col")
        assert_frame(bo, wb, f"{name} blackout_col")


def end_to_end(torch, scene, cam, W, H, k):
    scene.camera_uniform, scene.uniforms = camera_uniform(cam, W, H), uniforms()
    lens = torch.empty((k * H, k * W, 2), dtype=torch.float32, device="cuda")
    scene.render_lens(lens, width=k * W, height=k * H)
    for sky_name in SKIES:
        wc, wb = shade_mip_ref(cam, W, H, sky_name, k)
        col, bo = shade(torch, scene, lens, W, H, sky_name, ss=k)
        assert_frame(col, wc, f"{sky_name} col")
        assert_frame(bo, wb, f"{sky_name} blackout_col")
        if sky_name == "1x1":
            oc, ob = frame(cam, W, H, "1x1", k)
            assert_frame(col, oc, "1x1: the oracle's frame, col")
            assert_frame(bo, ob, "1x1: the oracle's frame, blackout_col")
        if sky_name == "96x40" and k == 1:
            plain = ~level_np(records(cam, W, H)[0], 96, 40)["filtered"]
            assert plain.any() and not plain.all()  # how many: test_census_of_the_reference (tests/test_lens_mip_host.py)
            oc, ob = frame(cam, W, H, "96x40")
            assert_frame(col, oc, "96x40: the oracle's pixels on the plain path, col", plain)
            assert_frame(bo, ob, "96x40: the oracle's pixels on the plain path, blackout_col", plain)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("cam", CAMS)
def test_end_to_end(torch_cuda, scene, cam, W, H):
    """render_lens on the GPU, then shade(mip=True): the reference of the oracle's records; with the 1x1 sky every
    byte is the oracle's frame, with 96x40 every pixel the reference puts on the plain path is the oracle's pixel."""
    end_to_end(torch_cuda, scene, cam, W, H, 1)


@pytest.mark.parametrize("cam", ["E", "H"])
def test_end_to_end_ss(torch_cuda, scene, cam):
    end_to_end(torch_cuda, scene, cam, 13, 7, 2)


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("fmt", [bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB])
def test_formats_and_col_alone(torch_cuda, scene, fmt, k):
    torch = torch_cuda
    W, H = (40, 24) if k == 1 else (13, 7)
    lens = upload(torch, records("E", W, H, k)[0])
    for sky_name in ("96x40", "512x256"):
        wc, wb = shade_mip_ref("E", W, H, sky_name, k)
        col, bo = shade(torch, scene, lens, W, H, sky_name, fmt, ss=k)
        assert_frame(col, expected_bytes(fmt, wc), f"{sky_name} fmt {fmt} col")
        assert_frame(bo, expected_bytes(fmt, wb), f"{sky_name} fmt {fmt} blackout_col")
        col, bo = shade(torch, scene, lens, W, H, sky_name, fmt, blackout=False, ss=k)  # out_blackout = NULL
        assert bo is None
        assert_frame(col, expected_bytes(fmt, wc), f"{sky_name} fmt {fmt} col alone")
    col, bo = shade(torch, scene, lens, W, H, "96x40", F32, blackout=False, ss=k)
    assert_frame(col, shade_mip_ref("E", W, H, "96x40", k)[0], "fp32 col alone")


def test_plain_shade_of_a_mipped_sky(torch_cuda, scene):
    """bh_shade_lens reads level 0 only: the bytes it gives with a plain sky of the same texels, the oracle's frame."""
    torch = torch_cuda
    W, H = 40, 24
    lens = upload(torch, records("E", W, H)[0])
    plain = bh.Sky(scene, sky("96x40"))
    try:
        col, bo = shade(torch, scene, lens, W, H, "96x40", mip=False)
        pc, pb = Target(torch, W, H, F32), Target(torch, W, H, F32)
        scene.shade(lens, pc.t, pb.t, sky=plain, width=W, height=H)
        torch.cuda.synchronize()
        assert np.array_equal(col, pc.bytes()) and np.array_equal(bo, pb.bytes())
        wc, wb = frame("E", W, H, "96x40")
        assert_frame(col, wc, "col")
        assert_frame(bo, wb, "blackout_col")
    finally:
        plain.close()


def test_no_state_between_shades(torch_cuda, scene):
    """One lens, the four skies back to back on one stream, then in reverse order: the same reference bytes."""
    torch = torch_cuda
    W, H = 40, 24
    lens = upload(torch, records("E", W, H)[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    for order in (SKIES, SKIES[::-1]):
        outs = {n: (Target(torch, W, H, F32), Target(torch, W, H, F32)) for n in order}
        for n in order:
            scene.shade(lens, outs[n][0].t, outs[n][1].t, sky=scene.mip_skies[n], width=W, height=H, stream=s, mip=True)
        s.synchronize()
        for n in SKIES:
            wc, wb = shade_mip_ref("E", W, H, n)
            assert_frame(outs[n][0].bytes(), wc, f"{n} col")
            assert_frame(outs[n][1].bytes(), wb, f"{n} blackout_col")


def test_graph(torch_cuda):
    """A filtered shade is capturable from its first call: a fresh scene's first bh_shade_lens_mip happens under
    capture on a single stream; replayed twice into sentinel-filled targets it gives the reference bytes."""
    torch = torch_cuda
    W, H = 40, 24
    sc = new_scene()
    try:
        sc.mip_skies = {"96x40": bh.Sky(sc, sky("96x40"), mips=True)}
        lens = upload(torch, records("E", W, H)[0])
        col, bo = Target(torch, W, H, F32), Target(torch, W, H, F32)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            sc.shade(lens, col.t, bo.t, sky=sc.mip_skies["96x40"], width=W, height=H, stream=s, mip=True)
        wc, wb = shade_mip_ref("E", W, H, "96x40")
        for _ in range(2):
            for t in (col, bo):
                t.whole.fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_frame(col.bytes(), wc, "replay: col")
            assert_frame(bo.bytes(), wb, "replay: blackout_col")
        del g
        sc.graph_release()
    finally:
        sc.close()


def test_refusals(torch_cuda, scene):
    torch = torch_cuda
    W, H = 40, 24
    lens = upload(torch, records("E", W, H)[0])
    big = torch.zeros((8 * H, 8 * W, 2), dtype=torch.float32, device="cuda")
    col, bo = Target(torch, W, H, F32), Target(torch, W, H, F32)
    stream = torch.cuda.current_stream().cuda_stream
    mipped = scene.mip_skies["96x40"]

    def desc(**kw):
        d = _abi.bh_shade_desc()
        d.width, d.height, d.ss, d.format = W, H, 1, F32
        d.lens, d.sky, d.out_col, d.out_blackout = lens.data_ptr(), mipped.handle, col.t.data_ptr(), bo.t.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    call = scene.lib.bh_shade_lens_mip
    other_scene = new_scene()
    chainless = bh.Sky(scene, sky("96x40"))
    try:
        foreign = bh.Sky(other_scene, sky("96x40"), mips=True)
        cases = [dict(sky=None), dict(sky=chainless.handle), dict(sky=foreign.handle),
                 dict(ss=0), dict(ss=3), dict(ss=16), dict(lens=None), dict(lens=lens.data_ptr() + 4), dict(out_col=None),
                 dict(width=0), dict(height=0), dict(width=32769, ss=2), dict(height=16385, ss=4), dict(width=65537),
                 dict(format=3), dict(ss=8, width=8193), dict(ss=8, sky=None)]
        for kw in cases:
            assert call(scene._ctx, C.byref(desc(**kw)), stream) == _abi.BH_ERR_INVALID_ARG, kw
        assert call(scene._ctx, None, stream) == _abi.BH_ERR_INVALID_ARG
        assert call(None, C.byref(desc()), stream) == _abi.BH_ERR_INVALID_ARG
        assert call(scene._ctx, C.byref(desc(ss=8, lens=big.data_ptr())), stream) == _abi.BH_ERR_UNSUPPORTED
        text = scene.lib.bh_last_error().decode()
        assert text.startswith("bh_shade_lens_mip") and text.endswith(".") and " " in text
        with pytest.raises(bh.BhError) as e:
            scene.shade(big, col.t, bo.t, sky=mipped, ss=8, width=W, height=H, mip=True)
        assert e.value.status == _abi.BH_ERR_UNSUPPORTED
        for bad_sky in (None, chainless):
            with pytest.raises(bh.BhError) as e:
                scene.shade(lens, col.t, bo.t, sky=bad_sky, width=W, height=H, mip=True)
            assert e.value.status == _abi.BH_ERR_INVALID_ARG
        lib = scene.lib
        n = C.c_uint32(7)
        assert lib.bh_sky_levels(None, C.byref(n)) == _abi.BH_ERR_INVALID_ARG and lib.bh_sky_levels(mipped.handle, None) == _abi.BH_ERR_INVALID_ARG
        assert lib.bh_sky_create_mips(None, sky("1x1").ctypes.data, 1, 1, C.byref(C.c_void_p())) == _abi.BH_ERR_INVALID_ARG
        assert lib.bh_sky_create_mips(scene._ctx, sky("1x1").ctypes.data, 0, 1, C.byref(C.c_void_p())) == _abi.BH_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert col.untouched() and bo.untouched()
        assert call(scene._ctx, C.byref(desc()), stream) == _abi.BH_OK  # the desc itself is good
        torch.cuda.synchronize()
        assert_frame(col.bytes(), shade_mip_ref("E", W, H, "96x40")[0], "col")
    finally:
        chainless.close()
        other_scene.close()


def test_render_path_tool(torch_cuda, tmp_path):
    """tools/render_path.py --sky-filter mip writes its frames, along a camera path and with --sky-frames and --ss;
    with --shutter or --adaptive it is refused."""
    tool = [sys.executable, str(ROOT / "tools" / "render_path.py"), "--sky-filter", "mip", "--width", "40", "--height", "24",
            "--max-iters", "64"]
    from black_hole_ray_marching_amd.png import write_png
    skies = tmp_path / "skies"
    skies.mkdir()
    for i, name in enumerate(("96x40", "512x256")):
        write_png(skies / f"sky_{i}.png", sky(name))
    out = tmp_path / "path"
    r = subprocess.run(tool + ["--frames", "2", "--ss", "2", "--sky", str(skies / "sky_1.png"), "--out", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"sky_filter": "mip"' in r.stdout
    assert sorted(p.name for p in out.glob("*.png")) == ["frame_0000.png", "frame_0001.png"]
    out = tmp_path / "sky"
    r = subprocess.run(tool + ["--sky-frames", str(skies), "--out", str(out)], capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(p.name for p in out.glob("*.png")) == ["frame_0000.png", "frame_0001.png"]
    for extra in (["--shutter", "2"], ["--ss", "2", "--adaptive", "0.05"], ["--ss", "8"]):  # refused before any GPU work
        r = subprocess.run(tool + extra + ["--out", str(tmp_path / "refused")], capture_output=True, text=True,
                           timeout=300, cwd=str(ROOT))
        assert r.returncode != 0 and "--sky-filter mip" in r.stderr, extra
    assert not (tmp_path / "refused").exists()
