"""Beamed disc shades on the CPU: bh_lens_shade_disc_beamed_host -- the functions of csrc/bh_lens.hpp the beamed shade
kernel runs -- against tests/_beam_ref.py's numpy restatement of include/bh_render.h's rule, bit for bit, over records
traced by the CPU oracle and over hand-made hits crossed with hand-made arrivals; the rule's three identities; the
conservation of E along the oracle's rays, which licenses forming it at the hit; the error returns that need no device."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests import _beam_ref as ref
from tests import _disc_ref as dref
from tests._ss_ref import sky_ss
from tests.test_disc_host import assert_same, edge_hits, edge_records

f32 = np.float32
RS, DP = float(ref.RS), float(ref.DP)
SURF = (bh.BH_LENS_SURFACE, 0.0)
BEAMS, SENSES, POWERS = (0.0, 0.5, 1.0), (1, -1), (0.0, 1.0, 2.5)


def check(rec, hits, arr, disc, k=1, **kw):
    """mirror == restatement for both targets"""
    got = bh.lens_shade_disc_beamed_host(rec, hits, arr, sky_ss(), disc, ss=k, rs=kw.get("rs", RS),
                                         scene_flags=kw.get("flags", 3), spin=kw.get("spin", 0.0), gain=kw.get("gain", 1.0),
                                         beam=kw.get("beam", 1.0), sense=kw.get("sense", 1),
                                         distortion_power=kw.get("dp", DP))
    want = ref.shade_ss(rec, hits, arr, sky_ss(), disc, k, **kw)
    assert_same(got[0], want[0], f"col {kw} ss {k}")
    assert_same(got[1], want[1], f"blackout_col {kw} ss {k}")
    return got


def test_the_symbols_are_there_and_the_abi_is_still_8():
    lib = bh.load()
    assert lib.bh_abi_version() == 8 == _abi.ABI_VERSION
    for name in ("bh_march_lens_arrivals", "bh_march_lens_rays_posed_arrivals", "bh_shade_lens_disc_beamed",
                 "bh_lens_shade_disc_beamed_host"):
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert len(_abi.SIGNATURES["bh_march_lens_arrivals"][1]) == len(_abi.SIGNATURES["bh_render_lens_hits"][1]) + 1
    assert len(_abi.SIGNATURES["bh_march_lens_rays_posed_arrivals"][1]) == len(_abi.SIGNATURES["bh_render_lens_rays_posed_hits"][1]) + 1
    assert len(_abi.SIGNATURES["bh_lens_shade_disc_beamed_host"][1]) == len(_abi.SIGNATURES["bh_lens_shade_disc_host"][1]) + 4
    assert C.sizeof(_abi.bh_beam_desc) == 24 and _abi.bh_beam_desc.distortion_power.offset == 16


@pytest.mark.parametrize("cam,W,H,cap", ref.FRAMES)
def test_mirror_equals_restatement_over_oracle_records(cam, W, H, cap):
    view = ref.pinhole_view(cam, W, H, cap)
    dref.assert_all_kinds(view[:3], f"{cam} {W}x{H} cap {cap}")
    ref.assert_both_sides(view, f"{cam} {W}x{H} cap {cap}")
    rec, _, hits, arr = view
    disc = dref.disc_texture(37, 5)
    for beam in BEAMS:
        for sense in SENSES:
            col, _ = check(rec, hits, arr, disc, spin=0.37, gain=4.0, beam=beam, sense=sense)
    for dp in POWERS:
        check(rec, hits, arr, disc, dp=dp)
    check(rec, hits, arr, disc, flags=2)  # without BH_SCENE_DISC every surface record is white, whatever its arrival
    # the beam is visible: the full factor moves disc hits both ways against the unbeamed shade
    on = ref.disc_mask(rec, hits)
    plain = bh.lens_shade_disc_host(rec, hits, sky_ss(), disc, rs=RS)[0]
    full = check(rec, hits, arr, disc)[0]
    lum = lambda c: c[..., :3].sum(-1)
    assert (lum(full)[on] > lum(plain)[on]).any() and (lum(full)[on] < lum(plain)[on]).any()
    assert np.array_equal(full[~on], plain[~on])


@pytest.mark.parametrize("k", [2, 4])
def test_mirror_equals_restatement_ss(k):
    cam, W, H, cap = "DISC_IN", 16, 8, 64
    rec, _, hits, arr = ref.pinhole_view(cam, W, H, cap, 3, k)
    for sense in SENSES:
        check(rec, hits, arr, dref.disc_texture(37, 5), k, spin=0.37, gain=4.0, beam=0.5, sense=sense)


def arrival_kinds(hits):
    """(15, 8, 8, 3): for each of the 64 hits p, arrivals tangential both ways, radial out and in, along +y and -y,
    zero, the first tangent at 1e18 and 1e-18, and the first tangent with a NaN, then an infinity, in each component"""
    x, y, z = (hits[..., c] for c in range(3))
    zero = np.zeros_like(x)
    tan = np.stack([-z, zero, x], -1)
    up = np.stack([zero, zero + f32(1), zero], -1)
    kinds = [tan, -tan, hits, -hits, up, -up, np.zeros_like(hits), tan * f32(1e18), tan * f32(1e-18)]
    for bad in (np.nan, np.inf):
        for c in range(3):
            a = tan.copy()
            a[..., c] = bad
            kinds.append(a)
    with np.errstate(all="ignore"):
        return np.stack(kinds).astype(f32)


def crossed():
    """(120, 8) records, hits and arrivals: the 64 hand-made hits under each kind of arrival, kind after kind"""
    hits = edge_hits()
    arr = arrival_kinds(hits)
    n = len(arr)
    return np.tile(edge_records(), (n, 1, 1)), np.tile(hits, (n, 1, 1)), arr.reshape(n * 8, 8, 3)


@pytest.mark.parametrize("n_phi,n_r", [(1, 1), (3, 2), (64, 16)])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_hand_made_hits_crossed_with_arrivals(n_phi, n_r, k):
    rec, hits, arr = crossed()
    disc = dref.disc_texture(n_phi, n_r)
    for beam in BEAMS:
        for sense in SENSES:
            for dp in POWERS:
                check(rec, hits, arr, disc, k, spin=0.37, gain=4.0, beam=beam, sense=sense, dp=dp)


@pytest.mark.parametrize("rs", [0.0, -1.0, 1e-30, float("nan"), float("inf")])
def test_every_rs_has_a_colour(rs):
    """rs is not validated: where a term of the factor is not finite, g = 1"""
    rec, hits, arr = crossed()
    with np.errstate(invalid="ignore"):
        scaled = hits * f32(rs if np.isfinite(rs) else 1.0)
    for h in (hits, scaled):
        for sense in SENSES:
            for beam in (0.5, 1.0):
                check(rec, h, arr, dref.disc_texture(3, 2), rs=rs, spin=-0.37, beam=beam, sense=sense)


def ring(lo=3.5, span=2.0, n=64):
    """(8, 8) surface records on the disc at rho = lo .. lo + span all the way round, with their prograde unit tangents"""
    phi = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    rho = lo + span * ((np.arange(n) * 7) % n) / n
    hits = np.stack([rho * np.cos(phi), 0.01 * np.cos(5 * phi), rho * np.sin(phi)], -1).astype(f32).reshape(8, 8, 3)
    tan = np.stack([-np.sin(phi), 0.0 * phi, np.cos(phi)], -1).astype(f32).reshape(8, 8, 3)
    return np.tile(np.asarray(SURF, f32), (8, 8, 1)), hits, tan


def test_an_arrival_tuned_to_a_negative_e2_keeps_the_colour():
    """A tangential arrival has h2 = r2 |d|^2, so E2 = |d|^2 (1 - dp rs / r): negative inside r = dp rs = 8."""
    rec, hits, tan = ring()
    _, g, E2, q, den = ref.factor_np(hits, tan, dp=8.0, parts=True)
    assert (E2 < 0).all() and (q > 0).all() and (g == 1).all()
    disc = dref.disc_texture(37, 5)
    got = check(rec, hits, tan, disc, dp=8.0, spin=0.37)
    want = bh.lens_shade_disc_host(rec, hits, sky_ss(), disc, rs=RS, spin=0.37)
    assert_same(got[0], want[0], "col")


def test_an_arrival_tuned_to_a_den_below_zero_keeps_the_colour():
    """The traced ray runs backwards: an arrival along the orbit is a photon that left against it, L.y < 0 for sense +1.
    At dp = 2.9 and rho in 3.05 .. 3.3, E is small and om |L.y| / E > 1.1: den <= 0 for the arrival against the orbit,
    den > 1 for the other."""
    rec, hits, tan = ring(3.05, 0.25)
    disc = dref.disc_texture(37, 5)
    plain = bh.lens_shade_disc_host(rec, hits, sky_ss(), disc, rs=RS)[0]
    for arr, sense in ((-tan, 1), (tan, -1)):
        _, g, E2, q, den = ref.factor_np(hits, arr, dp=2.9, sense=sense, parts=True)
        assert (E2 > 0).all() and (q > 0).all() and (den <= 0).all() and (g == 1).all()
        assert_same(check(rec, hits, arr, disc, dp=2.9, sense=sense)[0], plain, "col")
        _, g, _, _, den = ref.factor_np(hits, arr, dp=2.9, sense=-sense, parts=True)
        assert (den > 1).all() and (g < 1).all()
        check(rec, hits, arr, disc, dp=2.9, sense=-sense)


def test_identity_beam_zero_is_the_disc_shade():
    rng = np.random.Generator(np.random.PCG64(5))
    rec, _, hits, arr = ref.pinhole_view("DISC_IN", 16, 8, 64, 3, 2)
    hand = crossed()
    noise = lambda a: rng.standard_normal(a.shape).astype(f32)
    for r, h, a in ((rec, hits, arr), (rec, hits, noise(arr)), hand, (hand[0], hand[1], noise(hand[2]))):
        for k in (1, 2):
            for sense in SENSES:
                got = bh.lens_shade_disc_beamed_host(r, h, a, sky_ss(), dref.disc_texture(37, 5), rs=RS, spin=0.37, gain=4.0,
                                                     ss=k, beam=0.0, sense=sense, distortion_power=DP)
                want = bh.lens_shade_disc_host(r, h, sky_ss(), dref.disc_texture(37, 5), rs=RS, spin=0.37, gain=4.0, ss=k)
                assert_same(got[0], want[0], "col")
                assert_same(got[1], want[1], "blackout_col")


@pytest.mark.parametrize("cam,W,H,cap", ref.FRAMES)
def test_identity_scaling_every_arrival_by_a_power_of_two(cam, W, H, cap):
    """every op of steps 6 and 7 scales exactly: L by s, h2, E2 and dot(d, d) by s^2, E by s, L.y / E not at all"""
    rec, _, hits, arr = ref.pinhole_view(cam, W, H, cap)
    disc = dref.disc_texture(37, 5)
    kw = dict(rs=RS, spin=0.37, beam=1.0, sense=1, distortion_power=DP)
    want = bh.lens_shade_disc_beamed_host(rec, hits, arr, sky_ss(), disc, **kw)
    for s in (2.0, 0.5):
        got = bh.lens_shade_disc_beamed_host(rec, hits, arr * f32(s), sky_ss(), disc, **kw)
        assert_same(got[0], want[0], f"col, arrivals x {s}")
        assert_same(got[1], want[1], f"blackout_col, arrivals x {s}")


@pytest.mark.parametrize("cam,W,H,cap", ref.FRAMES)
def test_identity_flipping_the_sense_and_mirroring_z(cam, W, H, cap):
    """z -> -z of hits and arrivals negates L.y exactly and leaves r2, h2, E2 and rho alone; with the sense flipped too
    the factor is the same, and on a 1 x 1 white disc (no column to swap, weights that sum to 1) so are the bytes"""
    rec, _, hits, arr = ref.pinhole_view(cam, W, H, cap)
    flip = np.asarray([1, 1, -1], f32)
    kw = dict(rs=RS, spin=0.37, gain=0.5, beam=1.0, distortion_power=DP)
    for sense in SENSES:
        a = bh.lens_shade_disc_beamed_host(rec, hits, arr, sky_ss(), dref.white_disc(), sense=sense, **kw)
        b = bh.lens_shade_disc_beamed_host(rec, hits * flip, arr * flip, sky_ss(), dref.white_disc(), sense=-sense, **kw)
        assert_same(a[0], b[0], "col")
        assert_same(a[1], b[1], "blackout_col")
    c = bh.lens_shade_disc_beamed_host(rec, hits, arr, sky_ss(), dref.white_disc(), sense=1, **kw)
    assert not np.array_equal(a[0], c[0]), "the sense alone does change the frame"  # a: the last of the loop, sense -1


@pytest.mark.parametrize("cam,W,H,cap", [f for f in ref.FRAMES if f[0] in "AB"])
def test_energy_is_conserved_to_the_integrators_accuracy(cam, W, H, cap):
    """From the oracle alone, in f64: E at the hit against E at the camera, over the frame's disc hits.  Measured
    0.00099 (A) and 0.0011 (B); 0.005 leaves room for another libm and keeps the claim falsifiable."""
    drift = ref.energy_drift(cam, W, H, cap)
    print(f"{cam} {W}x{H} cap {cap}: max |E_hit / E_camera - 1| = {drift:.3g}")
    assert drift < 0.005


def test_host_mirror_refuses_invalid_arguments():
    lib = bh.load()
    rec, hits = np.ascontiguousarray(edge_records()), np.ascontiguousarray(edge_hits())
    arr = np.ascontiguousarray(arrival_kinds(hits)[0])
    sky, disc = np.ascontiguousarray(sky_ss()), np.ascontiguousarray(dref.disc_texture(3, 2))
    col, bo = np.empty((8, 8, 4), f32), np.empty((8, 8, 4), f32)

    def call(**kw):
        a = dict(lens=rec.ctypes.data, hits=hits.ctypes.data, w=8, h=8, ss=1, sky=sky.ctypes.data, sw=sky.shape[1],
                 sh=sky.shape[0], disc=disc.ctypes.data, n_phi=3, n_r=2, rs=RS, flags=3, spin=0.0, gain=1.0,
                 col=col.ctypes.data, bo=bo.ctypes.data, arr=arr.ctypes.data, beam=1.0, sense=1, dp=1.0)
        a.update(kw)
        return lib.bh_lens_shade_disc_beamed_host(a["lens"], a["hits"], a["w"], a["h"], a["ss"], a["sky"], a["sw"], a["sh"],
                                                  a["disc"], a["n_phi"], a["n_r"], a["rs"], a["flags"], a["spin"], a["gain"],
                                                  a["col"], a["bo"], a["arr"], a["beam"], a["sense"], a["dp"])

    assert call() == _abi.BH_OK and call(bo=None) == _abi.BH_OK and call(sense=-1, beam=0.0, dp=0.0) == _abi.BH_OK
    nan, inf = float("nan"), float("inf")
    for kw in (dict(lens=None), dict(hits=None), dict(sky=None), dict(disc=None), dict(col=None), dict(ss=3), dict(w=0),
               dict(n_phi=0), dict(n_r=32769), dict(flags=4), dict(spin=nan), dict(gain=-1.0), dict(gain=inf),
               dict(arr=None), dict(beam=-0.125), dict(beam=1.125), dict(beam=nan), dict(beam=inf), dict(sense=0),
               dict(sense=2), dict(sense=-2), dict(dp=nan), dict(dp=inf), dict(dp=-inf)):
        assert call(**kw) == _abi.BH_ERR_INVALID_ARG, kw
        assert lib.bh_last_error().decode().startswith("bh_lens_shade_disc_beamed_host:"), kw


def test_new_entry_points_refuse_null_arguments_by_name():
    """The three device entry points without a device: a NULL context is refused before any HIP call, a NULL or
    misaligned map with it, and the sentence names the function."""
    lib = bh.load()
    cam, U, d = _abi.bh_camera_uniform(), _abi.bh_uniforms(), _abi.bh_render_desc()
    pose, sd, dd, bd = _abi.bh_ray_pose(), _abi.bh_shade_desc(), _abi.bh_disc_desc(), _abi.bh_beam_desc()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ctx = C.c_void_p(p)  # never read: the pointer checks come first
    calls = {
        "bh_march_lens_arrivals": [
            lambda: lib.bh_march_lens_arrivals(None, C.byref(cam), C.byref(U), C.byref(d), p, p, p, None),
            lambda: lib.bh_march_lens_arrivals(ctx, C.byref(cam), C.byref(U), C.byref(d), p, p, None, None),
            lambda: lib.bh_march_lens_arrivals(ctx, C.byref(cam), C.byref(U), C.byref(d), p, p, p + 2, None),
            lambda: lib.bh_march_lens_arrivals(ctx, C.byref(cam), C.byref(U), C.byref(d), p, None, p, None),
            lambda: lib.bh_march_lens_arrivals(ctx, C.byref(cam), C.byref(U), C.byref(d), p + 4, p, p, None)],
        "bh_march_lens_rays_posed_arrivals": [
            lambda: lib.bh_march_lens_rays_posed_arrivals(None, C.byref(pose), C.byref(U), C.byref(d), p, p, p, p, None),
            lambda: lib.bh_march_lens_rays_posed_arrivals(ctx, C.byref(pose), C.byref(U), C.byref(d), p, p, p, None, None),
            lambda: lib.bh_march_lens_rays_posed_arrivals(ctx, C.byref(pose), C.byref(U), C.byref(d), p, p, p, p + 1, None),
            lambda: lib.bh_march_lens_rays_posed_arrivals(ctx, C.byref(pose), C.byref(U), C.byref(d), p, p, p + 1, p, None),
            lambda: lib.bh_march_lens_rays_posed_arrivals(ctx, C.byref(pose), C.byref(U), C.byref(d), None, p, p, p, None)],
        "bh_shade_lens_disc_beamed": [
            lambda: lib.bh_shade_lens_disc_beamed(None, C.byref(sd), C.byref(dd), C.byref(bd), None),
            lambda: lib.bh_shade_lens_disc_beamed(None, None, None, None, None)],
    }
    for name, fs in calls.items():
        for i, f in enumerate(fs):
            assert f() == _abi.BH_ERR_INVALID_ARG, (name, i)
            assert lib.bh_last_error().decode().startswith(name + ":"), (name, i, lib.bh_last_error())
