"""The host's side of the march waves' start (no GPU): the multiply-high magics a launch passes for its waves' two
divisions by launch constants (bh_common.hpp div_magic; bh_host.cpp fill_args)."""
import ctypes as C

import pytest

import black_hole_ray_marching_amd as bh


# ---- the magics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(1, 65), (65, 129), (129, 193), (193, 257)])
def test_magic_equals_division_for_every_slot(lo, hi):
    """Every divisor 1..256 and every dividend below 2^24: (n * magic) >> 32 == n / d, counted by the library's own
    loop over all of them; only d = 1 has no magic (its waves do not divide)."""
    lib = bh.load()
    n_max = (1 << 24) - 1
    for d in range(lo, hi):
        m = C.c_uint32(0)
        misses = lib.bh_div_magic_misses(d, n_max, C.byref(m))
        assert misses == 0, (d, m.value, misses)
        assert (m.value != 0) == (d > 1), (d, m.value)
        if d > 1:  # the library's count is of this arithmetic: spot-checked here against Python's integers
            for n in (0, 1, d - 1, d, d + 1, n_max - d, n_max - 1, n_max):
                assert (n * m.value) >> 32 == n // d, (d, n)


def test_magic_is_withheld_where_it_would_miss():
    """Beyond the range a magic is exact on, the host passes none (the wave divides): the bound n_max * e < 2^32 is
    the library's, and a magic it does pass never misses whatever the range (the headline's 2^22 slots by 32 frames,
    the largest launch's 2^32 - 16 slots by 255, a 16384-pixel-wide frame's tiles by its 2048 columns)."""
    lib = bh.load()
    m = C.c_uint32(0)
    assert lib.bh_div_magic_misses(32, (1 << 22) - 1, C.byref(m)) == 0 and m.value == (1 << 27) + 1
    assert lib.bh_div_magic_misses(3, 0xFFFFFFFF, C.byref(m)) == 0 and m.value == 0   # e = 2: exact below 2^31 only
    assert lib.bh_div_magic_misses(3, 1 << 26, C.byref(m)) == 0 and m.value == 0x55555556
    assert lib.bh_div_magic_misses(255, 0xFFFFFFEF, C.byref(m)) == 0 and m.value == 0
    assert lib.bh_div_magic_misses(2048, 2048 * 1024 - 1, C.byref(m)) == 0 and m.value == (1 << 21) + 1
    assert lib.bh_div_magic_misses(0, 5, C.byref(m)) < 0 and lib.bh_div_magic_misses(5, 5, None) < 0
