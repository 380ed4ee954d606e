"""The fast mode's f64 reference and noise yardstick (tests/_f64_ref.py), checked from the references alone: no GPU,
nothing of the code under test.  The f32 default path of oracle_np is what it was; straight rays have one fate in
f32 and f64; every case's allowance stays under the old envelope's 2 %; and noise of 2^-16 (about 100 ulp per
rd_derivative component) breaks the rule on the grazing cases, which is what the rule is for."""
import numpy as np
import pytest

from oracle import oracle_np
from tests import _f64_ref as F

TEETH = ["E", "B_rs8", "D_f0"]


@pytest.mark.parametrize("case_id", ["D_f3", "B_rs8"])
def test_the_f32_default_path_is_the_c_oracle(sky_small, case_id):
    """oracle_np with its defaults (float32, no noise) equals oracle/bh_oracle.c on every word: adding the scalar
    type and the noise hook changed nothing."""
    ref = F.reference(case_id, sky_small)
    c, b, n, f = oracle_np.render(ref.cu.pos, ref.cu.world_tri, ref.U.as_dict(), sky_small, ref.w, ref.h, ref.cap,
                                  ref.flags)
    oc, ob, on, of = ref.E_full
    assert c.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(f, of) and np.array_equal(n, on)
    assert np.array_equal(c.view(np.uint32), oc.view(np.uint32))
    assert np.array_equal(b.view(np.uint32), ob.view(np.uint32))


def test_noise_of_zero_is_the_default_path(sky_small):
    """The hook's f64 quotient rounded once is the f32 division: eps = 0 reproduces E bit for bit."""
    ref = F.reference("B_rs8", sky_small)
    c, n, f = ref.noisy(0, 0.0)
    assert np.array_equal(f, ref.E[2]) and np.array_equal(n, ref.E[1])
    assert np.array_equal(c.view(np.uint32), ref.E[0].view(np.uint32))


def test_the_f64_frame_is_f64_and_valid(sky_small):
    ref = F.reference("D_f3", sky_small)
    c, n, f = ref.R
    assert c.dtype == np.float64 and np.isfinite(c).all() and (c[..., 3] == 1).all()
    assert (c[..., :3] >= 0).all() and (c[..., :3] <= 1).all() and f.max() <= 3 and n.max() <= ref.cap
    assert set(np.unique(f)) >= {oracle_np.FATE_ESCAPE, oracle_np.FATE_SURFACE, oracle_np.FATE_BLACKOUT}


def test_straight_rays_have_one_fate_in_both_types(sky_small):
    """distortion_power = 0: no bending, nothing chaotic -- R's fates and n_rk equal E's everywhere."""
    ref = F.reference("B_dp0", sky_small)
    assert np.array_equal(ref.R[2], ref.E[2]) and np.array_equal(ref.R[1], ref.E[1])


@pytest.mark.parametrize("case_id", F.CASE_IDS)
def test_allowance_stays_under_two_percent(sky_small, case_id):
    """The cap that keeps the rule honest: 2 % of the frame is the old envelope's share."""
    ref = F.reference(case_id, sky_small)
    w, h = ref.w, ref.h
    print(f"{case_id} {w}x{h}: d(E) {ref.d_E}, d(N_i) {ref.d_N}, y {ref.y}, allowance {ref.allowance}")
    assert ref.allowance == 2 * max([ref.d_E] + ref.d_N) + 2
    assert ref.allowance <= 0.02 * w * h


@pytest.mark.parametrize("case_id", TEETH)
def test_the_rule_has_teeth(sky_small, case_id):
    """An error of about 100 ulp per division (noise 2^-16, a seed outside the ensemble) exceeds the allowance."""
    ref = F.reference(case_id, sky_small)
    got = ref.d(ref.noisy(99, 2.0 ** -16))
    print(f"{case_id}: d(noise 2^-16) {got}, allowance {ref.allowance}")
    assert got > ref.allowance
