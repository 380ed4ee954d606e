"""The scenario table (tests/_scenarios.py), host side (no GPU): every aim a scenario is in the table for is asserted
here from the CPU oracle alone, so that a scenario which silently stops exercising its aim cannot hide a hole in
tests/test_gpu_forms_matrix.py; and the library's host mirrors run over the new references."""
import functools

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
import oracle
from oracle import oracle_np
from tests import _adaptive_ref, _lens_ref, _rays_ref, _shutter_ref
from tests import _scenarios as S
from tests._cases import camera_uniform
from tests._ss_ref import DEFAULT, oracle_virtual, reference, scenario_uniforms, sky_ss

f32 = np.float32
CAP_, ESCAPE, SURFACE, BLACKOUT = bh.BH_FATE_CAP, bh.BH_FATE_ESCAPE, bh.BH_FATE_SURFACE, bh.BH_FATE_BLACKOUT
ALL_FATES = {CAP_, ESCAPE, SURFACE, BLACKOUT}
CYCLE_FIRST, CYCLE_END = 50, 192  # csrc/bh_march_ray.hpp: the first iteration a cycle can be seen at, CYCLE_ITERS_END


@functools.lru_cache(maxsize=None)
def dbg(sid: str, W: int, H: int, k: int = 1):
    """(n_rk, fate) of the scenario's virtual frame kW x kH"""
    s = S.BY_ID[sid]
    cu, U = camera_uniform(s.camera, W, H), scenario_uniforms(s.key)
    _, _, n_rk, fate = oracle.render_rows(cu.to_bytes(), bytes(U.to_c()), sky_ss(), k * W, k * H, s.cap, s.flags)
    return n_rk, fate


@functools.lru_cache(maxsize=None)
def cycling(sid: str, W: int, H: int, k: int = 1):
    """(ray, m): the first iteration m in CYCLE_FIRST..CYCLE_END-1 at which a ray's (ro, rd) equals its (ro, rd) at
    m - 2 bit for bit, for every ray of the virtual frame that has one: the state after m iterations is trace_ray's
    final state at max_iters = m.  Only a ray that ends at the cap can cycle."""
    s = S.BY_ID[sid]
    cu, U = camera_uniform(s.camera, W, H), bytes(scenario_uniforms(s.key).to_c())
    raw = np.frombuffer(cu.to_bytes(), f32)
    pos, tri = raw[0:3], raw[16:28].reshape(3, 4)[:, :3]
    dirs = oracle_np.pixel_dirs(tri, k * W, k * H)
    n_rk, fate = dbg(sid, W, H, k)
    out = []
    for i in np.flatnonzero((fate.ravel() == CAP_) & (n_rk.ravel() == s.cap)):
        def state(m):
            _, n, _, ro, rd = oracle.trace_ray(pos, dirs[i], U, sky_ss(), m, s.flags)
            assert n == m
            return np.concatenate([ro, rd]).view(np.uint32)
        back2, back1 = state(CYCLE_FIRST - 2), state(CYCLE_FIRST - 1)
        for m in range(CYCLE_FIRST, CYCLE_END):
            now = state(m)
            if np.array_equal(now, back2):
                out.append((int(i), m))
                break
            back2, back1 = back1, now
    return out


def reload_arm(sid, W, H, k=1):
    """the cycling rays that take the fast-forward's reload arm, (cap - m) & 1 == 1, and those that do not"""
    cap = S.BY_ID[sid].cap
    ms = [m for _, m in cycling(sid, W, H, k)]
    odd = sum((cap - m) & 1 for m in ms)
    return odd, len(ms) - odd


def arm_visible(sid, W, H, k=1):
    """The rays of the reload arm whose colour shows which of the cycle's two states the ray ends in: the colour at
    the cap differs from the colour one iteration earlier.  Few do: most cycles are fixed points (dt == 0), and the
    two states of camera E's 2-cycles differ in a component that the normalised direction does not keep."""
    s = S.BY_ID[sid]
    cu, U = camera_uniform(s.camera, W, H), bytes(scenario_uniforms(s.key).to_c())
    raw = np.frombuffer(cu.to_bytes(), f32)
    pos, tri = raw[0:3], raw[16:28].reshape(3, 4)[:, :3]
    dirs = oracle_np.pixel_dirs(tri, k * W, k * H)
    n = 0
    for i, m in cycling(sid, W, H, k):
        if (s.cap - m) & 1:
            a = oracle.trace_ray(pos, dirs[i], U, sky_ss(), s.cap, s.flags)[0]
            b = oracle.trace_ray(pos, dirs[i], U, sky_ss(), s.cap - 1, s.flags)[0]
            n += not np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return n


def test_default_scenario_is_the_existing_reference():
    a, b = reference("E", 40, 24, 2), reference("E", 40, 24, 2, scenario=DEFAULT)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)) and DEFAULT == (64, 3, ())


@pytest.mark.parametrize("sid", S.IDS)
def test_no_nan_or_inf_and_the_fates(sid):
    s = S.BY_ID[sid]
    for W, H in S.SIZES:
        for k in (1, 2):
            col, bo, _ = oracle_virtual(s.camera, W, H, k, s.key)
            assert np.isfinite(col).all() and np.isfinite(bo).all(), (W, H, k)
    seen = set(np.unique(dbg(sid, 40, 24)[1]).tolist())
    print(f"{sid}: fates {sorted(seen)} at 40x24")
    if sid in ("disc_F2", "mark_F2"):
        assert seen == ALL_FATES
    elif sid in ("none_E", "none_F2"):
        assert seen == {CAP_, ESCAPE, BLACKOUT}
    elif sid.startswith("big_s"):
        assert seen == {ESCAPE}
    else:
        assert len(seen) >= 2
    if s.flags == 0:
        assert SURFACE not in seen


def test_late_rays():
    """The plain loop behind CYCLE_ITERS_END, which no fast-forward can have shortened."""
    for sid, least in (("long_odd", 8), ("long_sat", 8)):
        n_rk, fate = dbg(sid, 40, 24)
        late = int(((n_rk >= CYCLE_END) & (fate != CAP_)).sum())
        print(f"{sid}: {late} rays end after iteration {CYCLE_END} with a fate other than CAP; "
              f"{int((n_rk >= CYCLE_END).sum())} reach it")
        assert late >= least


def test_cycling_rays():
    """long_odd: the reload arm (odd remainder), at ss 1 and ss 2; long_odd_none: the same in the Const<0> fold;
    long_sat: the other arm (even remainder)."""
    got = {(sid, k): reload_arm(sid, 40, 24, k) for sid, k in (("long_odd", 1), ("long_odd", 2), ("long_odd_none", 1),
                                                              ("long_sat", 1))}
    print("cycling rays (reload arm, other arm):", got)
    assert got[("long_odd", 1)][0] >= 2 and got[("long_odd", 2)][0] >= 2
    assert got[("long_odd_none", 1)][0] >= 8
    assert got[("long_sat", 1)][1] >= 2
    # what shows a wrong arm in a frame: observed 2 rays in long_odd_none at ss 2, none in long_odd (0 of 4 and of 23)
    seen = {(sid, k): arm_visible(sid, 40, 24, k) for sid, k in (("long_odd", 1), ("long_odd", 2), ("long_odd_none", 2))}
    print("rays whose colour depends on the arm:", seen)
    assert seen[("long_odd_none", 2)] >= 1


def test_gates():
    def of(sid):
        U = scenario_uniforms(S.BY_ID[sid].key)
        return S.gates(float(f32(U.rs)), float(f32(U.delta_time_mult)))
    assert of("none_E") == (True, True)          # the default uniforms: both on
    assert of("far_off") == (True, False)        # dtm 0.62: skip_sdf on, far_r2 = +inf
    assert of("rs8p2") == (False, False)         # rs > 8: skip_sdf off, so far_r2 = +inf
    assert of("rs8") == (True, True)             # rs == 8: the gate's upper edge, far_r2 finite
    assert of("big_s_f3") == (True, True)
    assert scenario_uniforms(S.BY_ID["bo0_E"].key).blackout_eh == 0 and scenario_uniforms().blackout_eh == 1


def test_saturated_cost():
    """min(steps >> 1, 255) saturates from 510 steps on: a tile of the launched frame holds such a ray."""
    for W, H, k in ((13, 7, 2), (40, 24, 1), (40, 24, 2)):
        n_rk, _ = dbg("long_sat", W, H, k)
        assert int((n_rk >= 510).sum()) >= 1, (W, H, k)
    assert int((dbg("long_odd", 40, 24)[0] >= 510).sum()) == 0


@pytest.mark.parametrize("sid", S.ADAPTIVE)
def test_adaptive_masks_are_mixed(sid):
    s = S.BY_ID[sid]
    W, H = S.ADAPTIVE_SIZE.get(sid, (40, 24))
    m = _adaptive_ref.tile_mask(bh.BH_OUT_RGBA32F, *_adaptive_ref.plain(s.camera, W, H, scenario=s.key), _adaptive_ref.T)
    print(f"{sid}: {int(m.sum())} of {m.size} tiles refined at {W}x{H}")
    assert 0 < int(m.sum()) < m.size
    col, bo = _adaptive_ref.composed(s.camera, W, H, S.ADAPTIVE_K.get(sid, 2), scenario=s.key)[:2]
    assert np.isfinite(col).all() and np.isfinite(bo).all()


@pytest.mark.parametrize("sid", S.SHUTTER)
def test_shutter_references_build(sid):
    """Every camera set of the shutter row is NaN-free (asserted by the builder) and holds at least two fates."""
    s = S.BY_ID[sid]
    for n, W, H in S.SHUTTER_SHAPES:
        cams = S.shutter_cameras(s, n, W, H)
        assert len(cams) == n and cams[0].to_bytes() == camera_uniform(s.camera, W, H).to_bytes()
        rc, rb = _shutter_ref.reference(cams, W, H, 1, s.key)
        assert np.isfinite(rc).all() and np.isfinite(rb).all()
        fates = np.concatenate([_shutter_ref.oracle_virtual(c, W, H, 1, s.key)[2].ravel() for c in cams])
        assert len(np.unique(fates)) >= 2


@pytest.mark.parametrize("sid", S.GENERAL_MAPS)
def test_general_maps_hold_two_fates(sid):
    s = S.BY_ID[sid]
    for name in S.GENERAL_POSITIONS:
        for W, H in S.SIZES:
            col, bo, rec, fate, _ = _rays_ref.general(name, W, H, s.key)
            assert not np.isnan(col).any() and len(np.unique(fate)) >= 2 and (s.flags != 0 or SURFACE not in fate)


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("sid", ["disc_F2", "long_odd"])
def test_host_mirrors_over_the_scenarios(sid):
    """bh_ss_resolve_host, bh_shutter_resolve_host, bh_lens_shade_host, bh_refine_mask_host and
    bh_ray_map_pinhole_host over the scenario's oracle frames equal the scenario's references bit for bit."""
    s = S.BY_ID[sid]
    W, H, k = 40, 24, 2
    col, bo, _ = oracle_virtual(s.camera, W, H, k, s.key)
    rc, rb = reference(s.camera, W, H, k, s.key)
    assert_bits(bh.ss_resolve_host(col, k), rc, "ss col")
    assert_bits(bh.ss_resolve_host(bo, k), rb, "ss blackout_col")
    assert not np.array_equal(rc, reference(s.camera, W, H, k)[0]), "the scenario's frame is not the default's"

    cams = S.shutter_cameras(s, 4, W, H)
    want = _shutter_ref.reference(cams, W, H, 1, s.key)
    for t in (0, 1):
        v = np.stack([_shutter_ref.oracle_virtual(c, W, H, 1, s.key)[t] for c in cams])
        assert_bits(bh.shutter_resolve_host(v, 4, 1)[0], want[t], f"shutter target {t}")

    rec, fate = _lens_ref.records(s.camera, W, H, 1, s.key)
    assert np.array_equal(fate, dbg(sid, W, H)[1])
    for sky_name in ("ctx", "96x40"):
        hc, hb = bh.lens_shade_host(rec, _lens_ref.sky(sky_name))
        wc, wb = _lens_ref.frame(s.camera, W, H, sky_name, 1, s.key)
        assert_bits(hc, wc, f"lens shade {sky_name} col")
        assert_bits(hb, wb, f"lens shade {sky_name} blackout_col")

    pc, pb = _adaptive_ref.plain(s.camera, W, H, scenario=s.key)
    assert np.array_equal(bh.refine_mask_host(pc, pb, bh.BH_OUT_RGBA32F, _adaptive_ref.T),
                          _adaptive_ref.tile_mask(bh.BH_OUT_RGBA32F, pc, pb, _adaptive_ref.T))

    tc, tb, trec, tfate, tn = _rays_ref.trace(_rays_ref.pinhole_map(s.camera, W, H), camera_uniform(s.camera, W, H).pos, s.key)
    oc, ob, _ = oracle_virtual(s.camera, W, H, 1, s.key)
    assert_bits(tc, oc, "pinhole map col")
    assert_bits(tb, ob, "pinhole map blackout_col")
    assert np.array_equal(trec.view(np.uint32), rec.view(np.uint32)) and np.array_equal(tn, dbg(sid, W, H)[0])
