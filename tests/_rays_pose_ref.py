"""Reference of the posed ray-map renders (bh_render_frames_rays, bh_render_frames_shutter_rays,
bh_render_lens_rays_posed) for tests/test_rays_pose_host.py and tests/test_gpu_rays_pose.py.  Never the GPU's own
output: for a camera-space map and a pose, ray by ray,

  the vector   the pose formula of include/bh_render.h restated in numpy fp32, every intermediate an np.float32 array
               and one rounding per operation, in the stated association: (mx r[c] + my u[c]) + mz f[c];
  the rest     tests/_rays_ref.trace of that world-space map from the pose's position: normalise, the CPU oracle's
               trace_ray, fs_main's blackout rule, the lens formula;
  ss > 1       tests/_ss_ref.resolve_np over the per-ray colours of the virtual frame's map;
  a shutter    tests/_shutter_ref.time_tree_np over the cameras' (resolved) frames.

Poses are named, so every trace is computed once per process and shared read-only."""
import functools

import numpy as np

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import raymap
from tests import _rays_ref as ref
from tests._rays_ref import DEFAULT, canonical_nan  # noqa: F401  (shared with the tests)
from tests._shutter_ref import time_tree_np
from tests._ss_ref import resolve_np

f32 = np.float32
ALL_FATES = {bh.BH_FATE_CAP, bh.BH_FATE_ESCAPE, bh.BH_FATE_SURFACE, bh.BH_FATE_BLACKOUT}


def _rot(forward, up):
    return np.stack(raymap.basis(forward, up)).astype(f32)


def _turn(i: int) -> np.ndarray:
    """An orthonormal basis that differs for every i: a view direction walking round the sphere, a tilted up."""
    a, b = 0.37 * i + 0.2, 0.23 * i - 0.4
    return _rot((np.cos(b) * np.sin(a), np.sin(b), np.cos(b) * np.cos(a)), (0.1 * np.sin(i), 1.0, 0.15))


# name -> (position name of _rays_ref.POSITIONS, the rows r, u, f as (3, 3) fp32)
NAMED = {
    "axesD": ("D", np.eye(3, dtype=f32)),                                           # the unit axes
    "rotH": ("H", _rot((3.0, 0.2, 1.0), (0.0, 1.0, 0.1))),                        # a rotated orthonormal basis
    "shearF2": ("F2", np.array([[1e-3, 2e-4, 0.0],                                  # sheared and scaled: rows of
                                [300.0, 900.0, -200.0],                             # lengths about 1e-3, 1e3 and 1
                                [0.3, -0.2, 0.9]], f32)),
    "mirrorD": ("D", _rot((-7.0, -1.5, 9.0), (0.0, 1.0, 0.0)) * np.array([[-1.0], [1.0], [1.0]], f32)),  # det -1
    "rotD": ("D", _rot((-7.0, -1.2, 9.5), (0.1, 1.0, 0.0))),
    "rotF2": ("F2", _rot((3.0, 1.0, 0.5), (0.0, 1.0, 0.0))),
}
POSES = list(NAMED)


def rows(name: str) -> np.ndarray:
    """(4, 3) fp32: pos, r, u, f of a named pose; "turn<i>" is the i-th generated rotation at position i % 3."""
    if name in NAMED:
        p, b = NAMED[name]
    else:
        i = int(name[len("turn"):])
        p, b = ref.POSITIONS[i % 3], _turn(i)
    out = np.concatenate([ref.position(p)[None, :], np.asarray(b, f32)]).astype(f32)
    assert out.shape == (4, 3) and np.isfinite(out).all()
    return out


def sequence(n: int, first: int = 0) -> tuple:
    """n distinct pose names from `first` on: the named ones -- the unit axes lead, so a set over a general map of D
    holds that map's own rays -- then generated turns."""
    names = POSES + [f"turn{i}" for i in range(256)]
    return tuple(names[first:first + n])


def apply_np(p: np.ndarray, m: np.ndarray) -> np.ndarray:
    """The pose formula in numpy fp32: (mx * r[c] + my * u[c]) + mz * f[c], each operation rounded once."""
    p, m = np.asarray(p, f32), np.asarray(m, f32)
    r, u, f = p[1], p[2], p[3]
    mx, my, mz = m[..., 0], m[..., 1], m[..., 2]
    out = np.empty(m.shape, f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            a = mx * r[c]
            b = my * u[c]
            ab = a + b
            cc = mz * f[c]
            out[..., c] = ab + cc
            assert a.dtype == b.dtype == ab.dtype == cc.dtype == f32
    return out


MAPS = {"general": lambda W, H: ref.general_map("D", W, H), "equirect": ref.equirect_map,
        "nonfinite": lambda W, H: ref.nonfinite_map()}


def camera_map(kind: str, W: int, H: int) -> np.ndarray:
    """The camera-space maps of the tests: "general" (row 0 the hand-made rays of position D, the rest the full
    sphere), "equirect", "nonfinite" (8 x 8)."""
    m = MAPS[kind](W, H)
    assert m.shape == (H, W, 3)
    return m


@functools.lru_cache(maxsize=None)
def posed(name: str, kind: str, W: int, H: int, scenario=DEFAULT):
    """_rays_ref.trace of the map turned by the pose, from the pose's position:
    (col, blackout_col, records, fate, n_rk)."""
    p = rows(name)
    return ref.trace(apply_np(p, camera_map(kind, W, H)), p[0], scenario)


def assert_all_fates(names, kind: str, W: int, H: int, what: str) -> None:
    """In the default scenario a test set reaches all four fates (over its poses together)."""
    seen = set()
    for n in names:
        seen |= set(np.unique(posed(n, kind, W, H)[3]).tolist())
    assert seen == ALL_FATES, f"{what}: fates {sorted(seen)}"


def frames(names, kind: str, W: int, H: int, k: int = 1):
    """[(col, blackout_col)] fp32 (H, W, 4), one per pose: the map of the virtual frame kW x kH, resolved."""
    out = []
    for n in names:
        col, bo = posed(n, kind, k * W, k * H)[:2]
        out.append((col, bo) if k == 1 else (resolve_np(col, k), resolve_np(bo, k)))
    return out


def shutter(names, kind: str, W: int, H: int, k: int = 1):
    """(col, blackout_col) fp32 (H, W, 4) of one output frame whose sub-frame cameras are `names`."""
    fs = frames(names, kind, W, H, k)
    return time_tree_np(np.stack([c for c, _ in fs])), time_tree_np(np.stack([b for _, b in fs]))
