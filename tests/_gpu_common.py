"""Helpers shared by the GPU parity tests: one render through the C ABI, the oracle's frame, the comparison."""
import numpy as np

import black_hole_ray_marching_amd as bh
import oracle

# the fast mode's colour tolerance (DESIGN.md "Math modes"), the one definition every fast-mode test imports.
# NOT the north_star 1e-4: a one-ulp change of the final ray direction moves the sky coordinate by ~2e-4
# texels, so at single-texel stars any non-bit-exact trajectory shows |delta| ~1e-3.
FAST_TOL = 5e-3

# every schedule, and both builds of the exact kernels (source order / machine-scheduled; the small
# test frames pick the latter by default)
SCHEDULES = [bh.BH_SCHED_PAIR, bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_ISSUE_ORDER,
             bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_LATENCY, bh.BH_SCHED_PERSISTENT | bh.BH_SCHED_FLAG_ISSUE_ORDER]


def gpu_render(torch, scene, cu, U, W, H, cap, flags, math, fmt=bh.BH_OUT_RGBA32F, blackout=True, schedule=0,
               steps=False):
    """(col, blackout or None, n_rk, fate) of one render, every target pre-filled with a pattern the kernel
    never writes; with steps=True also dbg_steps (the iterations actually executed) as a fifth array."""
    scene.camera_uniform = cu
    scene.uniforms = U
    scene.max_iters, scene.scene_flags = cap, flags
    ch_dtype = torch.float32 if fmt == bh.BH_OUT_RGBA32F else torch.float16
    col = torch.full((H, W, 4), float("nan"), dtype=ch_dtype, device="cuda")
    bo = torch.full((H, W, 4), float("nan"), dtype=ch_dtype, device="cuda") if blackout else None
    nrk = torch.full((H, W), 0xFFFF, dtype=torch.int32, device="cuda").to(torch.int16)
    fate = torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda")
    st = torch.full((H, W), 0xFFFF, dtype=torch.int32, device="cuda").to(torch.int16) if steps else None
    scene.render(col, bo, fmt=fmt, math=math, dbg_n_rk=nrk, dbg_fate=fate, dbg_steps=st, width=W, height=H,
                 schedule=schedule)
    torch.cuda.synchronize()
    out = (col.cpu().numpy(), None if bo is None else bo.cpu().numpy(),
           nrk.cpu().numpy().view(np.uint16), fate.cpu().numpy())
    return out + (st.cpu().numpy().view(np.uint16),) if steps else out


def oracle_render(cu, U, sky, W, H, cap, flags, row0=0, row1=None):
    return oracle.render_rows(cu.to_bytes(), bytes(U.to_c()), sky, W, H, cap, flags, row0, row1)


def assert_bitexact(g, o):
    gc, gb, gn, gf = g
    oc, ob, on, of = o
    assert np.array_equal(gf, of), f"fate mismatch at {np.argwhere(gf != of)[:5]}"
    assert np.array_equal(gn, on), f"n_rk mismatch at {np.argwhere(gn != on)[:5]}"
    bad = gc.view(np.uint32) != oc.view(np.uint32)
    assert not bad.any(), f"col mismatch at {np.argwhere(bad)[:5]}: {gc[bad][:4]} vs {oc[bad][:4]}"
    if gb is not None:
        assert np.array_equal(gb.view(np.uint32), ob.view(np.uint32))


def bgra8_expected(col_f32):
    """The Bgra8UnormSrgb bytes of an fp32 colour: the normative encode (oracle bho_srgb_encode), alpha 255."""
    enc = oracle.srgb_encode(col_f32[..., :3])
    out = np.empty(col_f32.shape[:-1] + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = enc[..., 2], enc[..., 1], enc[..., 0], 255
    return out
