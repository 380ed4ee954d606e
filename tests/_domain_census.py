"""Which steps of a frame leave the domains of the exact kernels' correctly rounded cores.  TEST INFRASTRUCTURE.

census() replays a frame with oracle_np's own arithmetic (its get_col, observed step by step: nothing of the
integrator is restated here) and counts, over the rays that take each RK step, the steps on which a guard
condition of the march holds.  A step that leaves a domain must raise the kernel's `bad` and re-run in plain
IEEE ops; the edge table of tests/_cases.py is tuned until these counts show that it does (test_edge_inputs.py).

The thresholds are the C++ constants by value.  If one of them moves, this file moves with it:
"""
import numpy as np

from oracle import oracle_np as onp

f32 = np.float32

DIV_D_MIN = f32(2.0 ** -40)    # bh_crmath.hpp  crm::DIV_D_MIN  (div_d_bad: Q = (q*q)*sqrt(q) >= 2^-40)
DIV_D_MAX = f32(2.0 ** 60)     # bh_crmath.hpp  crm::DIV_D_MAX  (div_d_bad: Q <= 2^60)
ACC_N_MIN = f32(2.0 ** -40)    # bh_crmath.hpp  crm::ACC_N_MIN / KEY_ACC_MIN  (step_bf: kmin, amin)
DIV_N_MIN = f32(2.0 ** -60)    # bh_crmath.hpp  crm::DIV_N_MIN  (step_bf: amin6, the x/6 numerators)
SQRT_MIN = f32(2.0 ** -96)     # bh_crmath.hpp  crm::SQRT_MIN   (sqrt_bad, sqrt_bad2)
DT_MIN = f32(2.0 ** -25)       # bh_march_step.hpp   step_bf, "rd_half's premise": |dt| >= 0x1p-25f or dt == 0
S_MAX = f32(2.0 ** 30)         # bh_march_step.hpp   step_bf / the pair step; bh_march_tile.hpp march_slot's ballot: |s| <= 0x1p30f

COUNTERS = ("q_hi", "q_lo", "n_lo", "n6_lo", "dt_tiny", "dt_zero", "dt_neg", "root_lo", "nonfinite")


def _any(masks):
    out = masks[0].copy()
    for m in masks[1:]:
        out |= m
    return out


def census(cam_pos, world_tri, U, W, H, cap, flags):
    """Per pixel ((H, W) int64 arrays) and in total, the number of RK steps of alive rays on which
      q_hi / q_lo   one of the four stage denominators Q is above 2^60 / below 2^-40,
      n_lo          a non-zero acceleration numerator s * p_i is below 2^-40 in magnitude,
      n6_lo         a non-zero x/6 numerator is below 2^-60 in magnitude,
      dt_tiny / dt_zero / dt_neg   0 < |dt| < 2^-25 / dt == 0 / dt < 0,
      root_lo       the argument of one of the step's square roots is below 2^-96,
      nonfinite     the state going in, dt or a stage denominator is not finite;
    and s_big, per ray (bool (H, W)): !(|s| <= 2^30), the per-ray constant of rd_derivative.
    Returns (per_pixel: dict, total: dict, frame: oracle_np.render's result)."""
    n = W * H
    per = {k: np.zeros(n, np.int64) for k in COUNTERS}
    s_big = np.zeros(n, bool)
    sky = np.zeros((2, 2, 4), np.uint8)  # colours are not the census's business

    def observe(alive, s, ro, rd, dt, cps, stages, sums):
        s_big[:] = ~(np.abs(s) <= S_MAX)
        qs = [onp._dot(*p, *p) for p in stages]
        Qs = [onp._pow25(q) for q in qs]
        nums = [s * c for p in stages for c in p]
        roots = list(qs)
        roots.append(onp._dot(*(c - p for c, p in zip(cps, ro)), *(c - p for c, p in zip(cps, ro))))
        if flags & onp.SCENE_DISC:
            roots.append(ro[0] * ro[0] + ro[2] * ro[2])
        if flags & onp.SCENE_MARKERS:
            for c in ((0.0, 10.0, -10.0), (0.0, -10.0, -10.0), (10.0, 0.0, -10.0), (-10.0, 0.0, -10.0)):
                d = tuple(f32(ck) - pk for ck, pk in zip(c, ro))
                roots.append(onp._dot(*d, *d))
        state = list(ro) + list(rd) + [dt] + Qs
        hit = {
            "q_hi": _any([Q > DIV_D_MAX for Q in Qs]),
            "q_lo": _any([Q < DIV_D_MIN for Q in Qs]),
            "n_lo": _any([(v != 0) & (np.abs(v) < ACC_N_MIN) for v in nums]),
            "n6_lo": _any([(v != 0) & (np.abs(v) < DIV_N_MIN) for v in sums]),
            "dt_tiny": (dt != 0) & (np.abs(dt) < DT_MIN),
            "dt_zero": dt == 0,
            "dt_neg": dt < 0,
            "root_lo": _any([v < SQRT_MIN for v in roots]),
            "nonfinite": _any([~np.isfinite(v) for v in state]),
        }
        for k, m in hit.items():
            per[k] += alive & m

    with np.errstate(all="ignore"):
        frame = onp.render(cam_pos, world_tri, U, sky, W, H, cap, flags, observe=observe)
    per = {k: v.reshape(H, W) for k, v in per.items()}
    per["s_big"] = s_big.reshape(H, W)
    total = {k: int(v.sum()) for k, v in per.items()}
    return per, total, frame


def s_big_tiles(s_big):
    """(tiles with lanes on both sides of 2^30, tiles wholly above it) over the frame's 8x8 tiles, partial
    tiles included: the two cases of march_slot's per-wave ballot that choose the general step."""
    H, W = s_big.shape
    mixed = full = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            t = s_big[ty:ty + 8, tx:tx + 8]
            mixed += bool(t.any() and not t.all())
            full += bool(t.all())
    return mixed, full
