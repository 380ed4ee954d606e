"""CPU tests of the edge table (tests/_cases.py EDGE_CASES): the oracle is well defined on every input the
reference's unclamped key bindings reach, and each case reaches the guard it aims at.

The GPU half is tests/test_gpu_edge_inputs.py.  Here: oracle/bh_oracle.c equals the numpy restatement bit for
bit on the whole table, and the census of tests/_domain_census.py -- the oracle alone, no kernel -- shows for
every declared counter at least MIN_STEPS ray-steps outside the core's domain.  That is a condition, not a
measurement: it keeps a later edit of a camera from turning a case into one that tests nothing."""
import numpy as np
import pytest

import oracle
from oracle import oracle_np
from tests._cases import (DTM_RESIDUE, EDGE_AIMS, EDGE_CASES, EDGE_IDS, RS_RESIDUE, camera_uniform, pressed,
                          uniforms)
from tests._domain_census import COUNTERS, census, s_big_tiles

MIN_STEPS = 64


def test_pressed_reproduces_the_key_press_residues():
    f32 = np.float32
    # the residues as printed, to the digits quoted (8, 8, 7 and 7 significant)
    assert "%.8g" % pressed(1, .2, -5) == "2.9802322e-08" and RS_RESIDUE == pressed(1, .2, -5) > 0
    assert "%.8g" % pressed(1, .2, -6) == "-0.19999997"
    assert "%.7g" % pressed(.5, .02, -25) == "-8.940697e-08" and DTM_RESIDUE == pressed(.5, .02, -25) < 0
    assert "%.7g" % pressed(.5, .02, -26) == "-0.02000009"
    for n in (-5, -6):
        assert f32(pressed(1, .2, n)) == pressed(1, .2, n)  # every result is an f32
    # the two sides of the gates the table names
    assert f32(pressed(1, .2, +36)) > f32(8) and abs(pressed(1, .2, +36) - 8.2) < 1e-4
    assert abs(pressed(1, .2, -4) - 0.2) < 1e-6
    assert abs(pressed(.5, .02, +6) - 0.62) < 1e-6 and abs(pressed(.5, .02, +5) - 0.60) < 1e-6
    # sequential additions, not value + n * inc
    assert pressed(1, .2, -5) != float(f32(1) - f32(5) * f32(.2))
    assert pressed(3.0, .5, 0) == 3.0


def test_edge_table_shape():
    assert len(set(EDGE_IDS)) == len(EDGE_IDS) == len(EDGE_CASES)
    for i, (cam, W, H, cap, flags, over) in zip(EDGE_IDS, EDGE_CASES):
        assert W <= 44 and H <= 28 and cap <= 256, i
        assert set(EDGE_AIMS[i]) <= set(COUNTERS) | {"s_big", "clear"}, i


@pytest.mark.parametrize("cam,W,H,cap,flags,over", EDGE_CASES, ids=EDGE_IDS)
def test_oracle_is_defined_and_reaches_its_guard(sky_small, request, cam, W, H, cap, flags, over):
    cu, U = camera_uniform(cam, W, H), uniforms(**over)
    col, bo, n_rk, fate = oracle.render_rows(cu.to_bytes(), bytes(U.to_c()), sky_small, W, H, cap, flags)
    with np.errstate(all="ignore"):
        c2, b2, n2, f2 = oracle_np.render(cu.pos, cu.world_tri, U.as_dict(), sky_small, W, H, cap, flags)
    assert np.array_equal(fate, f2) and np.array_equal(n_rk, n2)
    assert np.array_equal(col.view(np.uint32), c2.view(np.uint32))
    assert np.array_equal(bo.view(np.uint32), b2.view(np.uint32))
    assert np.isfinite(col).all() and (col[..., 3] == 1).all()
    assert np.isfinite(bo).all() and (bo[..., 3] == 1).all()
    assert fate.max() <= 3 and n_rk.max() <= cap

    per, total, frame = census(cu.pos, cu.world_tri, U.as_dict(), W, H, cap, flags)
    assert np.array_equal(frame[2], n_rk) and np.array_equal(frame[3], fate)  # the census replayed this frame
    for aim in EDGE_AIMS[request.node.callspec.id]:
        if aim == "clear":
            assert not any(total.values()), total
        elif aim == "s_big":
            # march_slot's ballot: a wave with lanes on both sides of 2^30, and one wholly above it
            mixed, full = s_big_tiles(per["s_big"])
            assert mixed >= 1 and full >= 1, (mixed, full)
            assert not per["s_big"].all()
        else:
            assert total[aim] >= MIN_STEPS, (aim, total)


def test_edge_cases_do_what_their_group_says(sky_small):
    """The fates the table's comments promise, from the oracle: frozen rays cap, a max_dist of 0 or below
    lets every ray escape after one step, rs = NaN blacks every ray out after one, the origin camera's rays
    are NaN from step 1 and shade texel (0, 0)."""
    from tests._cases import EDGE

    def run(i):
        cam, W, H, cap, flags, over = EDGE[i]
        cu, U = camera_uniform(cam, W, H), uniforms(**over)
        return oracle.render_rows(cu.to_bytes(), bytes(U.to_c()), sky_small, W, H, cap, flags), cap

    (col, _, n_rk, fate), cap = run("dtm_zero")
    assert (fate == oracle_np.FATE_CAP).all() and (n_rk == cap).all()
    for i in ("max_dist_zero", "max_dist_negative"):
        (col, _, n_rk, fate), cap = run(i)
        assert (fate == oracle_np.FATE_ESCAPE).all() and (n_rk == 1).all()
    (col, _, n_rk, fate), cap = run("rs_nan")
    assert (fate == oracle_np.FATE_BLACKOUT).all() and (n_rk == 1).all() and (col[..., :3] == 0).all()
    lut = oracle.srgb_lut()
    t = lut[sky_small[0, 0, :3]]
    texel = np.array([t[0], t[1] * np.sqrt(t[1]), t[2] * np.sqrt(t[2])], np.float32)
    for i in ("origin_bo0", "origin_bo1"):
        (col, _, n_rk, fate), cap = run(i)
        assert (fate == oracle_np.FATE_CAP).all() and (n_rk == cap).all()
        assert np.array_equal(col[..., :3].view(np.uint32), np.broadcast_to(texel, col[..., :3].shape).view(np.uint32))
    (col, _, n_rk, fate), cap = run("near3_bo1")
    assert (fate[n_rk == 0] == oracle_np.FATE_BLACKOUT).all() and (n_rk == 0).sum() > 100  # ingoing: black at once
    assert (fate == oracle_np.FATE_ESCAPE).sum() > 100                                      # outgoing rays march
