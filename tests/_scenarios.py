"""The scenario table of the derived march kernels (supersampled, adaptive, shutter, lens, ray map, ray-map lens):
the points of the plain march's input space -- scene-flag fold, cap, uniform gates -- that tests/test_gpu_forms_matrix.py
renders each derived form at, and whose aims tests/test_scenarios_host.py asserts from the CPU oracle alone.

A scenario is (id, camera of tests/_cases.py, cap, flags, uniform overrides, aims); its `key` (cap, flags, overrides) is
the `scenario` argument of the reference builders (tests/_ss_ref.py DEFAULT = (64, 3, ()): overrides as a sorted
tuple of (name, value) pairs, so the key is hashable and the builders' per-process caches hold it)."""
from typing import NamedTuple

from tests._cases import EDGE, pressed
from tests._ss_ref import DEFAULT


class Scenario(NamedTuple):
    id: str
    camera: str
    cap: int
    flags: int
    overrides: tuple
    aims: str

    @property
    def key(self):
        return (self.cap, self.flags, self.overrides)


def _s(id, camera, cap, flags, aims, **overrides):
    return Scenario(id, camera, cap, flags, tuple(sorted(overrides.items())), aims)


_BIG_S = EDGE["big_s_f3"][5]  # the edge table's: rs = 8, distortion_power = 6, max_dist = 20000
assert _BIG_S == EDGE["big_s_f0"][5]

# The adaptive row (ADAPTIVE below) holds the scenarios whose numpy mask at T = 0.1 is mixed (refined and unrefined
# tiles: tests/test_scenarios_host.py asserts it) at 40x24, or, bo0_E (15 of 15 tiles refined at 40x24), at 44x27 (23
# of 24).  rs8 is left out of the row: camera B with rs = 8 refines every tile at both sizes.
TABLE = [
    _s("none_E", "E", 64, 0, "Const<0> fold, camera-outside step, capped rays"),
    _s("none_F2", "F2", 64, 0, "Const<0> fold, general step (camera inside the unit sphere)"),
    _s("disc_F2", "F2", 64, 1, "SF_DYN, disc only; all four fates at 40x24"),
    _s("disc_D", "D", 64, 1, "SF_DYN, camera-outside step"),
    _s("mark_F2", "F2", 64, 2, "SF_DYN, markers only; all four fates at 40x24"),
    _s("mark_B", "B", 64, 2, "SF_DYN, far camera"),
    _s("long_odd", "E", 257, 3, "loop past iteration 192; the fast-forward's reload arm"),
    _s("long_odd_none", "E", 257, 0, "the same in the Const<0> fold"),
    _s("long_sat", "E", 600, 3, "even remainder; saturated tile costs in the learned order"),
    _s("bo0_E", "E", 257, 3, "no blackout: rays reach r ~ 0; blackout_col differs from col only by the dot test",
       blackout_eh=0),
    _s("far_off", "A", 64, 3, "far_r2 = +inf", delta_time_mult=pressed(.5, .02, +6)),
    _s("rs8", "B", 64, 3, "the skip_sdf gate's upper edge", rs=8.0),
    _s("rs8p2", "D", 64, 3, "skip_sdf off", rs=pressed(1, .2, +36)),
    _s("big_s_f3", "BIGS", 64, 3, "march_slot's per-wave choice falls to the general step at abs(s) > 2^30", **_BIG_S),
    _s("big_s_f0", "BIGS", 64, 0, "the same in the Const<0> fold", **_BIG_S),
]
IDS = [s.id for s in TABLE]
BY_ID = {s.id: s for s in TABLE}
assert len(BY_ID) == len(TABLE) == 15 and DEFAULT not in [s.key for s in TABLE]

SIZES = [(13, 7), (40, 24)]   # partial tiles on both axes; whole and partial tiles
LONG = ["long_odd", "long_odd_none", "long_sat"]
# the rows of the GPU matrix that do not take every scenario
ADAPTIVE = ["none_E", "disc_F2", "mark_F2", "long_odd", "long_odd_none", "bo0_E"]
ADAPTIVE_K = {"disc_F2": 4}   # k = 2 otherwise
ADAPTIVE_SIZE = {"bo0_E": (44, 27)}   # 40 x 24 otherwise
SHUTTER = ["none_F2", "disc_F2", "mark_B", "long_odd", "long_sat", "bo0_E", "far_off"]
SHUTTER_SHAPES = [(2, 13, 7), (16, 13, 7), (4, 40, 24)]
# with ss = 2; long_odd_none at 40x24, where two rays' colour depends on the reload arm (tests/test_scenarios_host.py)
SHUTTER_SS = [("disc_F2", 4, 13, 7), ("long_odd", 4, 13, 7), ("long_odd_none", 2, 40, 24)]
SS_K4 = ["none_E", "disc_F2", "long_odd"]
SS_K8 = ["mark_F2"]
MIP = ["disc_F2", "long_odd"]
GENERAL_MAPS = ["none_E", "none_F2", "disc_F2", "disc_D", "mark_F2", "mark_B", "long_odd"]
GENERAL_POSITIONS = ["F2", "D"]
RAYS_SS = ["disc_F2", "long_odd"]
LENS_RAYS = ["none_F2", "disc_F2", "mark_F2", "long_odd"]
FORMATS = ["none_E", "disc_F2", "long_odd"]
FAST = ["none_E", "disc_F2"]


def gates(rs: float, dtm: float):
    """(skip_sdf, far_r2 is finite): the host's decision in fill_args and sdf_far_r2 (csrc/bh_host.cpp)."""
    skip = dtm > 0.0 and 0.0 < rs <= 8.0
    far = skip and 0.5 ** 0.5 - 1.1251 * dtm > 0.01
    return skip, far


def shutter_cameras(s: Scenario, n: int, W: int, H: int):
    """The scenario's camera as camera 0, then tests/_shutter_ref.MIXED cycled: the waves of one workgroup take both
    the camera-outside and the general step."""
    from tests._cases import camera_uniform
    from tests._shutter_ref import mixed
    return (camera_uniform(s.camera, W, H),) + mixed(n - 1, W, H)
