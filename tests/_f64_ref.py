"""The fast mode's reference: an f64 frame, and the f32 references' own sensitivity to one ulp as the yardstick.

BH_MATH_FAST promises no bits, and near the photon sphere the step map is chaotic: an ulp becomes another
step count, fate or exit direction.  A mismatch against the f32 oracle therefore cannot tell a differently
rounded trajectory from a subtly wrong kernel -- the f32 oracle is itself one rounding of that map.  So, per case:

  R    the f64 frame: oracle_np's statements with every input and literal at its f32 value, promoted;
  E    the exact f32 frame (the C oracle);
  N_i  eight f32 frames in which every rd_derivative result carries relative noise of 2^-23 (seed i = 0..7);
  d(X) the number of pixels on which X leaves R: fate or n_rk differs, or R's ray is not capped and
       max over RGB of |X - R| >= FAST_TOL;
  y = max(d(E), d(N_0..7)),  allowance = 2 y + 2.

The yardstick never involves the code under test.  The factor 2: a ninth exchangeable draw exceeds the maximum
of eight with probability 1/9, and the fast build perturbs more than rd_derivative (the roots of dt and of the
sdf, FMA contraction); twice the maximum leaves the ensemble's spread far behind and stays well under what an
error of ~100 ulp per division produces (tests/test_f64_ref_host.py shows both ends).  The + 2 is the existing
bar's "or at most 2 pixels differ".
"""
import numpy as np

from oracle import oracle_np
from tests._cases import camera_uniform, uniforms
from tests._gpu_common import FAST_TOL, oracle_render

W, H = 100, 52      # 13 x 7 = 91 tiles, an odd count, partial tiles on both edges
N_NOISE = 8
NOISE_EPS = 2.0 ** -23

# Two cases take a larger frame, also of an odd tile count with partial tiles on both edges, because at 100x52 the
# real cameras leave them too few sensitive pixels for the rule to notice noise of 2^-16 (test_f64_ref_host.py
# "the rule has teeth": 5 <= 6 for E, 0 <= 2 for D_f0): camera E's shadow edge runs down the frame, so its frame
# grows in height (7 x 25 tiles); D_f0 doubles (25 x 13 tiles).
# id -> (camera, W, H, cap, flags, uniform overrides), as test_gpu_parity.CASES
CASES = {
    "A": ("A", W, H, 512, 3, {}),
    "D_f3": ("D", W, H, 512, 3, {}),
    "D_f0": ("D", 200, 100, 512, 0, {}),
    "D_f1": ("D", W, H, 512, 1, {}),
    "D_f2": ("D", W, H, 512, 2, {}),
    "C_cap1000": ("C", W, H, 1000, 3, {}),
    "E": ("E", 52, 196, 512, 3, {}),
    "B_rs8": ("B", W, H, 512, 3, {"rs": 8.0}),
    "A_bo0": ("A", W, H, 512, 3, {"blackout_eh": 0}),
    "B_dp0": ("B", W, H, 512, 3, {"distortion_power": 0.0}),
}
CASE_IDS = list(CASES)


def differing(x, r):
    """The mask of d(X): x and r are (col, n_rk, fate) triples (col of any float type, alpha ignored)."""
    xc, xn, xf = x
    rc, rn, rf = r
    delta = np.abs(xc[..., :3].astype(np.float64) - rc[..., :3].astype(np.float64)).max(axis=-1)
    with np.errstate(invalid="ignore"):
        far = ~(delta < FAST_TOL)           # a NaN colour counts as a difference
    return (xf != rf) | (xn.astype(np.int64) != rn.astype(np.int64)) | ((rf != oracle_np.FATE_CAP) & far)


def d(x, r):
    return int(differing(x, r).sum())


class Ref:
    """One frame's references; every array is read-only."""

    def __init__(self, cu, U, w, h, cap, flags, sky):
        self.cu, self.U, self.w, self.h, self.cap, self.flags, self.sky = cu, U, w, h, cap, flags, sky
        self._args = (cu.pos, cu.world_tri, U.as_dict(), sky, w, h, cap, flags)
        self.R = self._np(dtype=np.float64)
        c, b, n, f = oracle_render(cu, U, sky, w, h, cap, flags)
        self.E_full = _frozen((c, b, n, f))
        self.E = (c, n, f)
        self.N = [self._np(noise=(i, NOISE_EPS)) for i in range(N_NOISE)]
        self.d_E = d(self.E, self.R)
        self.d_N = [d(x, self.R) for x in self.N]
        self.y = max([self.d_E] + self.d_N)
        self.allowance = 2 * self.y + 2

    def _np(self, **kw):
        with np.errstate(over="ignore", invalid="ignore"):  # stage positions of rays plunging to r ~ 0 overflow r^5
            c, _, n, f = oracle_np.render(*self._args, **kw)
        return _frozen((c, n, f))

    def noisy(self, seed, eps):
        """An f32 frame with relative noise eps on every rd_derivative result (not cached)."""
        return self._np(noise=(seed, eps))

    def d(self, x):
        return d(x, self.R)


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


_cache = {}


def reference_of(cu, U, w, h, cap, flags, sky):
    """The Ref of the w x h frame of camera uniform cu (which may belong to another frame size: a supersampled
    render's virtual frame), built once per session and shared.  One sky per session: conftest.sky_small."""
    key = (cu.to_bytes(), bytes(U.to_c()), w, h, cap, flags)
    if key not in _cache:
        _cache[key] = Ref(cu, U, w, h, cap, flags, sky)
    assert _cache[key].sky is sky or np.array_equal(_cache[key].sky, sky)
    return _cache[key]


def reference(case_id, sky):
    """The Ref of a case of CASES."""
    cam, w, h, cap, flags, over = CASES[case_id]
    return reference_of(camera_uniform(cam, w, h), uniforms(**over), w, h, cap, flags, sky)
