"""The guard form of k1's numerators in the loop behind the peeled first step (csrc/bh_march_ops.hpp XOps<true, true>)
against the key test it replaces there (csrc/bh_crmath.hpp key), both restated in numpy on the bit patterns.  A guard
only decides whether a step re-runs in IEEE ops, so the replacement must fire at least where the old one fired:

  the float test, min |n| >= 2^-40 over fminf, fires wherever the key test fires, and besides it only where a
  component is +-0 (the known cost: a ray in a coordinate plane re-runs) -- or where all three components are NaN:
  fminf drops a NaN operand, so one or two NaNs among the three are dropped by the float chain and mapped high by
  the key alike, and three leave NaN, which fails `>=`.  The k2..k4 chain has always fired there; the division is
  NaN either way.

The constants are read from the header, so the restatement cannot drift from it.  (The pooled range test of the three
stage denominators, which this file also held to div_d_bad, measured slower and is not in the tree: DESIGN.md §5 item 35.)"""
import re
from pathlib import Path

import numpy as np

f32, u32 = np.float32, np.uint32
CRMATH = (Path(__file__).resolve().parent.parent / "black_hole_ray_marching_amd" / "csrc" / "bh_crmath.hpp").read_text()


def header_f32(name):
    return f32(float.fromhex(re.search(rf"constexpr float {name} = (\S+?)f;", CRMATH).group(1)))


ACC_N_MIN = header_f32("ACC_N_MIN")
KEY_ACC_MIN = (int(re.search(r"KEY_ACC_MIN = \((0x[0-9A-Fa-f]+)u << 1\) - 1u;", CRMATH).group(1), 16) << 1) - 1


def bits(x):
    return np.ascontiguousarray(x, f32).view(u32)


def bits1(x):
    return int(bits(f32(x)).reshape(-1)[0])


def from_bits(u):
    return np.ascontiguousarray(u, u32).view(f32)


def around(x, n):
    """The n floats below x, x, and the n floats above it."""
    b = bits1(x)
    return from_bits(np.arange(b - n, b + n + 1, dtype=np.int64).astype(u32))


def test_header_constants():
    assert ACC_N_MIN == f32(2.0 ** -40)
    assert KEY_ACC_MIN == 2 * bits1(ACC_N_MIN) - 1


# ---- k1's numerators: the float chain against the key --------------------------------------------------------------------
def key_fires(nx, ny, nz):
    k = [((bits(n).astype(np.uint64) << 1) - 1) & 0xFFFFFFFF for n in (nx, ny, nz)]   # crm::key, mod 2^32
    return np.minimum(np.minimum(k[0], k[1]), k[2]) < KEY_ACC_MIN


def float_fires(nx, ny, nz):
    amin = np.fmin(np.fmin(np.abs(nx), np.abs(ny)), np.abs(nz))   # XOps::absmin3: fminf drops a NaN operand
    with np.errstate(invalid="ignore"):
        return ~(amin >= ACC_N_MIN)


def numerators():
    return np.concatenate([
        around(ACC_N_MIN, 3), -around(ACC_N_MIN, 3),
        from_bits([0x00000000, 0x80000000]),
        from_bits([0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x00400000]),
        from_bits([0x7FC00000, 0xFFC00000, 0x7FFFFFFF]),
        np.array([2.0 ** -60, 2.0 ** -61, -2.0 ** -126, 1.0, -3.0, 2.0 ** 42, np.inf, -np.inf], f32),
    ])


def test_float_numerator_test_covers_the_key_test():
    v = numerators()
    nx, ny, nz = (x.ravel() for x in np.meshgrid(v, v, v, indexing="ij"))
    key, flt = key_fires(nx, ny, nz), float_fires(nx, ny, nz)
    assert key.any() and (~flt).any()
    assert not (key & ~flt).any(), "the key test fires where the float test does not"
    extra = flt & ~key
    has_zero = (nx == 0) | (ny == 0) | (nz == 0)
    all_nan = np.isnan(nx) & np.isnan(ny) & np.isnan(nz)
    assert extra.any() and not (extra & ~(has_zero | all_nan)).any()
    # every triple with a zero component is such an extra fire unless the key fires too (a tiny value beside the zero)
    assert np.array_equal(extra | key, flt) and (flt[has_zero]).all()
    print(f"float test fires on {int(flt.sum())} of {flt.size} triples, the key test on {int(key.sum())}; "
          f"{int(extra.sum())} more: {int((extra & has_zero).sum())} with a +-0 component, "
          f"{int((extra & ~has_zero).sum())} all-NaN")
    assert int((extra & ~has_zero).sum()) == 3 ** 3   # the three NaN patterns in every position


def test_float_numerator_test_covers_the_key_test_on_random_patterns():
    rng = np.random.default_rng(26)
    e = rng.integers(127 - 44, 127 - 36, size=(3, 1 << 20), dtype=np.uint64)      # around 2^-40
    m = rng.integers(0, 1 << 23, size=(3, 1 << 20), dtype=np.uint64)
    sgn = rng.integers(0, 2, size=(3, 1 << 20), dtype=np.uint64) << 31
    n = [from_bits((s | (ee << 23) | mm).astype(u32)) for s, ee, mm in zip(sgn, e, m)]
    key, flt = key_fires(*n), float_fires(*n)
    assert np.array_equal(key, flt) and 0.05 < key.mean() < 0.95   # no zero, no NaN: the same test
    u = rng.integers(0, 1 << 32, size=(3, 1 << 20), dtype=np.uint64).astype(u32)
    n = [from_bits(x) for x in u]
    key, flt = key_fires(*n), float_fires(*n)
    assert not (key & ~flt).any()
