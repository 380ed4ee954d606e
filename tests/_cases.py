"""Shared parity cases: cameras A/B/C, uniforms variants, frame sizes."""
import numpy as np

import black_hole_ray_marching_amd as bh

CAMERAS = {
    "A": None,                                   # Scene::new default, src/scene.rs:68-76
    "B": ((0.0, 3.0, -20.0), (0.0, 0.0, 0.0)),
    "C": ((0.0, 6.0, -12.0), (0.0, 0.0, 0.0)),
    "D": ((7.0, 1.5, -9.0), (0.0, 0.0, 0.0)),    # off-axis, close: many disc/photon-sphere rays
    "E": ((0.0, 0.0, -20.0), (2.6, 0.0, 0.0), 0.1),  # zoom on the shadow edge: capped "Zeno" rays
    # the camera at the unit sphere (the blackout test's two clauses, :272-283; the kernel's
    # camera-outside step applies for |pos|^2 > 1.01 only, bh_march_step.hpp SF_CAM_OUT):
    "F": ((0.0, 0.0, -0.5), (0.0, 0.0, -5.0)),   # inside, looking out: escapes, caps and blackouts
    "F2": ((0.2, 0.1, -0.5), (3.0, 1.0, 0.0)),   # inside, sideways: also disc hits
    "G": ((0.0, 0.6, -0.8018), (4.0, 0.6, -0.8)),  # |pos|^2 = 1.0029: outside, general step
    "H": ((0.0, 0.0, -1.02), (3.0, 0.0, -1.0)),  # |pos|^2 = 1.0404: camera-outside step, rays plunge in
    # the edge table's cameras (EDGE_CASES below): where the reference's keys O and P (exponential motion
    # away from / towards the origin) take the camera within seconds
    "FAR": ((0.0, 500.0, -6000.0), (0.0, 0.0, 0.0), 0.02),   # r = 6021: Q = r^5 > 2^60, hole in view
    "FARW": ((0.0, 500.0, -6000.0), (0.0, 0.0, 0.0)),        # ... with the default fov
    "R3000": ((0.0, 300.0, -2985.0), (0.0, 0.0, 0.0)),       # r = 3000: far field, inside every domain
    "BIGS": ((0.0, 500.0, -6000.0), (3000.0, 0.0, 0.0)),     # r = 6021 aimed off the hole: |ro x rd|^2 ~ 1e7
    "IN03": ((0.0, 0.0, -0.3), (0.0, 0.0, -5.0)),            # r = 0.3 looking outward
    "NEAR3": ((0.0, 0.0, -3e-3), (1.0, 0.2, -3e-3)),         # r = 3e-3 looking sideways: Q = r^5 < 2^-40
    "NEAR5": ((0.0, 0.0, -3e-5), (1.0, 0.2, -3e-5)),         # r = 3e-5
    "ORIGIN": ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0)),            # exactly at the origin: normalize(0) = NaN
}


def camera_uniform(name: str, width: int, height: int) -> bh.CameraUniform:
    spec = CAMERAS[name]
    cam = bh.Camera.default(width, height) if spec is None else bh.Camera.look_at(spec[0], spec[1], width, height)
    if spec is not None and len(spec) > 2:
        cam.fovy = spec[2]
    cu = bh.CameraUniform()
    cu.update(cam)
    return cu


def uniforms(**kw) -> bh.Uniforms:
    u = bh.Uniforms.default()
    for k, v in kw.items():
        setattr(u, k, v)
    return u


def pressed(value, inc, n):
    """The f32 that |n| key presses leave: n sequential f32 additions of +inc (n > 0) or -inc (n < 0), as the
    reference's IncValue::increment / decrement do (src/otheruniforms.rs) -- not value + n * inc."""
    v, d = np.float32(value), np.float32(inc if n > 0 else -inc)
    for _ in range(abs(n)):
        v = np.float32(v + d)
    return float(v)


# ---- the edge table: uniforms and cameras the reference's key bindings reach, unclamped -----------------
# rs moves by +-0.2, delta_time_mult by +-0.02, distortion_power by +-0.2, max_dist by +-1 (src/scene.rs:89-137).
RS_RESIDUE = pressed(1, .2, -5)        # 2.9802322e-08: above 0, so the root-free gate stays on
DTM_RESIDUE = pressed(.5, .02, -25)    # -8.940697e-08
_W, _H = 44, 28                        # partial tiles on both edges
_NEXT8 = float(np.nextafter(np.float32(8), np.float32(np.inf)))
_NAN, _INF = float("nan"), float("inf")

# (id, the census counters the case aims at (tests/_domain_census.py; "clear" = no guard may fire), case);
# a case is (camera, W, H, cap, flags, uniform overrides) like test_gpu_parity.CASES
_EDGE = [
    # far: Q > 2^60 (crm::DIV_D_MAX), the IEEE re-run on most steps, the far-field step at large magnitudes
    ("far_narrow", ("q_hi",), ("FAR", _W, _H, 256, 3, {"max_dist": 20000.0})),
    ("far_wide", ("q_hi",), ("FARW", _W, _H, 256, 3, {"max_dist": 20000.0})),
    ("far_r3000", ("clear",), ("R3000", _W, _H, 256, 3, {})),
    ("far_r3000_long", ("clear",), ("R3000", _W, _H, 256, 3, {"delta_time_mult": pressed(.5, .02, -20), "max_dist": 1000.0})),
    # big_s: |s| > 2^30 and march_slot's per-wave choice of the SF_CAM_OUT step (fixed-flag instantiations)
    ("big_s_f3", ("s_big", "q_hi"), ("BIGS", _W, _H, 256, 3, {"rs": 8.0, "distortion_power": 6.0, "max_dist": 20000.0})),
    ("big_s_f0", ("s_big", "q_hi"), ("BIGS", _W, _H, 256, 0, {"rs": 8.0, "distortion_power": 6.0, "max_dist": 20000.0})),
]
# rs: the host's gate 0 < rs <= 8 and sdf_far_r2
for _cam in ("B", "D"):
    for _name, _rs in (("residue", RS_RESIDUE), ("zero", 0.0), ("negative", pressed(1, .2, -6)),
                       ("0p2", pressed(1, .2, -4)), ("8p2", pressed(1, .2, +36)), ("next8", _NEXT8)):
        _EDGE.append((f"rs_{_name}_{_cam}", (), (_cam, _W, _H, 256, 3, {"rs": _rs})))
_EDGE += [
    # dtm: dt == 0, dt < 0, the gate dtm > 0, the far-field switch at ~0.62, 0 < |dt| < 2^-25
    ("dtm_zero", ("dt_zero",), ("B", _W, _H, 256, 3, {"delta_time_mult": 0.0})),
    ("dtm_residue", ("dt_neg",), ("B", _W, _H, 256, 3, {"delta_time_mult": DTM_RESIDUE})),
    ("dtm_negative", ("dt_neg",), ("B", _W, _H, 256, 3, {"delta_time_mult": pressed(.5, .02, -26)})),
    ("dtm_0p62", (), ("A", _W, _H, 256, 3, {"delta_time_mult": pressed(.5, .02, +6)})),
    ("dtm_0p60", (), ("A", _W, _H, 256, 3, {"delta_time_mult": pressed(.5, .02, +5)})),
    ("dtm_residue_in_bo0", ("dt_tiny", "dt_neg"), ("IN03", _W, _H, 256, 3, {"delta_time_mult": DTM_RESIDUE, "blackout_eh": 0})),
    ("dtm_residue_in_bo1", ("dt_tiny", "dt_neg"), ("IN03", _W, _H, 256, 3, {"delta_time_mult": DTM_RESIDUE, "blackout_eh": 1})),
    # near: Q < 2^-40, numerators below 2^-40 and 2^-60, root arguments below 2^-96
    ("near3_f0", ("q_lo", "n6_lo", "q_hi"), ("NEAR3", _W, _H, 256, 0, {"blackout_eh": 0})),
    ("near3_f3", ("q_lo", "n6_lo", "q_hi"), ("NEAR3", _W, _H, 256, 3, {"blackout_eh": 0})),
    ("near5_f0", ("q_lo", "n_lo", "n6_lo", "q_hi"), ("NEAR5", _W, _H, 256, 0, {"blackout_eh": 0, "delta_time_mult": 0.1})),
    ("near5_f3", ("q_lo", "n_lo", "n6_lo", "q_hi"), ("NEAR5", _W, _H, 256, 3, {"blackout_eh": 0, "delta_time_mult": 0.1})),
    ("near3_bo1", ("q_lo", "n6_lo", "q_hi"), ("NEAR3", _W, _H, 256, 3, {"blackout_eh": 1})),
    # other reachable states
    ("dp_repulsive", (), ("B", _W, _H, 256, 3, {"distortion_power": pressed(1, .2, -7)})),
    ("max_dist_zero", (), ("B", _W, _H, 256, 3, {"max_dist": 0.0})),
    ("max_dist_negative", (), ("B", _W, _H, 256, 3, {"max_dist": -1.0})),
    # non-finite: the ABI promises a status, never an abort, and the oracle defines every output
    ("origin_bo0", ("nonfinite", "root_lo", "q_lo"), ("ORIGIN", _W, _H, 32, 3, {"blackout_eh": 0})),
    ("origin_bo1", ("nonfinite", "root_lo", "q_lo"), ("ORIGIN", _W, _H, 32, 3, {"blackout_eh": 1})),
    ("rs_nan", (), ("B", _W, _H, 16, 3, {"rs": _NAN})),
    ("max_dist_inf", ("q_hi", "nonfinite"), ("B", _W, _H, 64, 3, {"max_dist": _INF})),
]
EDGE_IDS = [e[0] for e in _EDGE]
EDGE_AIMS = {e[0]: e[1] for e in _EDGE}
EDGE_CASES = [e[2] for e in _EDGE]
EDGE = dict(zip(EDGE_IDS, EDGE_CASES))
