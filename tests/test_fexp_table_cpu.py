"""The pair kernels' table exp with the biased table (csrc/mm_device.h: fexp_scale, fexp_finish; csrc/pair.hip:
mm_exp_table_fill), checked on the CPU: the integer identity behind the exponent insertion for every table index over the
whole range of n the -700 clamp allows, and the emulated exp against the previous formulation (unbiased table, exponent
inserted after the final FMA) bit for bit.  The FMA is emulated exactly with fractions.Fraction (CPython's int / int
true division rounds correctly)."""
import struct
from fractions import Fraction

import numpy as np

TB = 8
TN = 1 << TB
C = float(TN) * 1.4426950408889634074
LN2_T = 0.69314718055994530942 / float(TN)
MAGIC = 6755399441055744.0


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _dbl(u):
    return struct.unpack("<d", struct.pack("<Q", u & 0xFFFFFFFFFFFFFFFF))[0]


def _hi(x):
    return _bits(x) >> 32


def _lo(x):
    return _bits(x) & 0xFFFFFFFF


def _hilo(hi, lo):
    return _dbl(((hi & 0xFFFFFFFF) << 32) | (lo & 0xFFFFFFFF))


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _tables():
    tab = [float(np.exp2(j / TN)) for j in range(TN)]
    btab = [_hilo(_hi(v) - (j << (20 - TB)), _lo(v)) for j, v in enumerate(tab)]   # mm_exp_table_fill
    return tab, btab


def _poly(x, t):
    nf = t - MAGIC
    r = fma(nf, -LN2_T, x)
    q = fma(r, 1.0 / 24.0, 1.0 / 6.0)
    q = fma(r, q, 0.5)
    q = fma(r, q, 1.0)
    return r * q


def fexp_old(x, tab):
    x = max(x, -700.0)
    t = fma(x, C, MAGIC)
    tv = tab[_lo(t) & (TN - 1)]
    res = fma(tv, _poly(x, t), tv)
    lo = _lo(t) & ~(TN - 1) & 0xFFFFFFFF
    return _hilo(_hi(res) + (lo << (20 - TB)), _lo(res))


def fexp_new(x, btab):
    x = max(x, -700.0)
    t = fma(x, C, MAGIC)
    tvb = btab[_lo(t) & (TN - 1)]
    tv = _hilo(_hi(tvb) + (_lo(t) << (20 - TB)), _lo(tvb))   # fexp_scale
    return fma(tv, _poly(x, t), tv)


def test_biased_entry_plus_shifted_n_is_scaled_entry_exactly():
    """For every index j and every n = 256 m + j in [-258 600, 65 536] (x >= -700 gives n >= -258 530): the biased
    high word plus n << 12 equals tab_hi[j] + (m << 20) as a 32-bit integer, negative n and n = 0 mod 256 included."""
    tab, btab = _tables()
    n = np.arange(-258600, 65537, dtype=np.int64)
    j = n & (TN - 1)
    m = n >> TB                                                     # floor division: n = 256 m + j
    hi = np.array([_hi(v) for v in tab], dtype=np.int64)
    bhi = np.array([_hi(v) for v in btab], dtype=np.int64)
    lo = n & 0xFFFFFFFF                                             # the low word of t = 1.5 2^52 + n
    got = (bhi[j] + (lo << (20 - TB))) & 0xFFFFFFFF
    want = (hi[j] + (m << 20)) & 0xFFFFFFFF
    assert np.array_equal(got, want)
    # the low words are the table's own
    assert all(_lo(a) == _lo(b) for a, b in zip(tab, btab))


def test_emulated_exp_matches_previous_formulation_bitwise():
    tab, btab = _tables()
    rs = np.random.RandomState(7)
    xs = list(rs.uniform(-700.0, 700.0, 1500)) + list(rs.uniform(-30.0, 5.0, 800))
    # around n = 0 mod 256 (r changing sign at the table's ends), the clamp, below it, and around every power of two
    # boundary of the result near the origin
    for k in range(-4, 5):
        c0 = k * 256 * LN2_T
        xs += [c0 + d for d in (-0.6 * LN2_T, -1e-9, 0.0, 1e-9, 0.6 * LN2_T)]
    xs += [-700.0, -699.999, -700.5, -720.0, -5000.0, 0.0, -0.0, 1e-300, 700.0]
    for j in range(TN):
        xs.append((j + 0.49) * LN2_T)
        xs.append(-(j + 0.51) * LN2_T - 3 * 256 * LN2_T)
    for x in xs:
        a, b = fexp_old(float(x), tab), fexp_new(float(x), btab)
        assert _bits(a) == _bits(b), (x, a, b)
    # and it is the exp
    for x in xs[:200]:
        x = max(float(x), -700.0)
        assert abs(fexp_new(x, btab) / np.exp(x) - 1.0) < 2.3e-16 + 1.2e-16 * abs(x)
