"""The lemma behind the ESIM step's quotient screen, checked in exact arithmetic on the CPU.

The step computes u = p * inv with inv = fl(1 / C) * (1 - 2^-51) (biased low), q = trunc(u) and -- before the screen, in every step --
r = fma(-q, C, p); it ran the +1 fix-up when !(|r| < C).  The screen runs that test only when the top 24 bits of u's low 32-bit word are
all ones.  Claim: for finite p and C with |u| < 2^20, whenever the old test fires the screen passes.  `fractions.Fraction` gives the
correctly rounded fma (float(Fraction) rounds to nearest even).

Second claim: clip parameters that pass the kernel's bound expression keep |u| below 2^20 at the largest potential they admit
(|p| <= max(C+, C-) + 7.0 + 4.0625 * (base_std + hot_std): the reset leaves |potential| < C, a table-valued log difference is at
most log(1.001) - log(0.001) = 6.909, a deviate of the Gaussian table at most 4.009)."""
import math
import random
import struct
from fractions import Fraction

INV_BIAS = float.fromhex("0x1.ffffffffffffcp-1")      # the kernel's one-sided correction of the reciprocal
LOG_SPREAD, GAUSS_MAX = 7.0, 4.0625                    # kScreenLogSpread, kScreenGaussMax of v2v_esim.hpp
TWO20 = float(1 << 20)


def lo32(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] & 0xFFFFFFFF


def inv_low(c):
    return (1.0 / c) * INV_BIAS


def step(p, c):
    """(u, old test fires, screen passes) of one pixel-step, the kernel's operations in the kernel's order."""
    u = p * inv_low(c)
    q = float(math.trunc(u))
    r = float(Fraction(p) - Fraction(q) * Fraction(c))          # fma(-q, C, p), correctly rounded
    return u, not (abs(r) < c), (lo32(u) >> 8) == 0xFFFFFF


def bound_passes(c_pos, c_neg, base_std, hot_std):
    """The kernel's expression, operation by operation (quotient_bound_num and the compare against 2^20 * min)."""
    noise = GAUSS_MAX * (base_std + hot_std)
    reach = max(c_pos, c_neg) + LOG_SPREAD
    return (reach + noise) < TWO20 * min(c_pos, c_neg)


def smallest_admissible(noise_std):
    """Smallest symmetric threshold that passes the bound with base_std + hot_std = noise_std."""
    c = (LOG_SPREAD + GAUSS_MAX * noise_std) / (TWO20 - 1.0)
    while bound_passes(c, c, noise_std, 0.0):
        c = math.nextafter(c, 0.0)
    while not bound_passes(c, c, noise_std, 0.0):
        c = math.nextafter(c, math.inf)
    return c


def thresholds():
    g = random.Random(20240611)
    cs = [0.2, 0.3, 0.05, 1.0] + [g.uniform(1e-3, 2.0) for _ in range(200)]
    # the extremes the bound admits: the smallest threshold without noise (about 7 * 2^-20), its upper neighbours, and the largest (1e30)
    c0 = smallest_admissible(0.0)
    return cs + [c0, math.nextafter(c0, math.inf), 1.5 * c0, 1e30]


def multipliers():
    g = random.Random(7)
    return list(range(1, 70)) + [g.randrange(70, 1 << 19) for _ in range(60)]


def test_old_test_fires_only_behind_the_screen():
    cases = fixups = 0
    ns = multipliers()
    for c in thresholds():
        for n in ns:
            centre = n * c
            ps = [centre]
            lo = hi = centre
            for _ in range(6):
                lo, hi = math.nextafter(lo, 0.0), math.nextafter(hi, math.inf)
                ps += [lo, hi]
            for p in ps:
                for s in (p, -p):
                    u, fires, screen = step(s, c)
                    assert abs(u) < TWO20, (c, n, s)
                    cases += 1
                    if fires:
                        fixups += 1
                        assert screen, f"fix-up missed: C={c.hex()} n={n} p={s.hex()} u={u.hex()}"
    # not vacuous: exact multiples and their upper neighbours do need the fix-up (a first version counted 127,574 of 700,986)
    print(f"{cases} cases, {fixups} fix-ups, none missed")
    assert cases > 600_000 and fixups > cases // 10


def test_screen_is_rare_on_ordinary_quotients():
    """The screen passes for 2^-24 of random quotients: none of 20,000 seeded draws, so the rare branch stays rare."""
    g = random.Random(3)
    hits = sum(step(g.uniform(-8.0, 8.0), g.uniform(1e-3, 2.0))[2] for _ in range(20_000))
    assert hits == 0


def extreme_u(c_pos, c_neg, base_std, hot_std):
    """u at the largest potential the parameters admit, rounded up, over the smaller threshold."""
    p = float(Fraction(max(c_pos, c_neg)) + Fraction(6.909) + Fraction(4.009) * (Fraction(base_std) + Fraction(hot_std)))
    p = math.nextafter(math.nextafter(p, math.inf), math.inf)
    return p * inv_low(min(c_pos, c_neg))


def test_bound_expression_keeps_the_quotient_below_2_pow_20():
    g = random.Random(11)
    passed = refused = 0
    rows = []
    for _ in range(4000):
        c_pos = 10.0 ** g.uniform(-9.0, 30.0)
        c_neg = c_pos if g.random() < 0.5 else c_pos * 10.0 ** g.uniform(-7.0, 7.0)
        c_neg = min(max(c_neg, 1e-9), 1e30)
        std = [0.0, 0.0] if g.random() < 0.3 else [10.0 ** g.uniform(-4.0, 6.0), 10.0 ** g.uniform(-4.0, 6.0)]
        rows.append((c_pos, c_neg, std[0], std[1]))
    # the edge itself, with and without noise: the smallest admissible threshold and its neighbours on either side
    for noise in (0.0, 0.1, 0.2, 1.0, 1e3):
        c = smallest_admissible(noise)
        for _ in range(4):
            c = math.nextafter(c, 0.0)
        for _ in range(9):
            rows.append((c, c, noise, 0.0))
            rows.append((c, 1.7 * c, 0.0, noise))
            c = math.nextafter(c, math.inf)
    rows += [(0.2, 0.2, 0.1, 0.1), (0.2, 0.3, 0.1, 0.1), (1e-6, 1e-6, 1.0, 0.1), (1e30, 1e30, 1e30, 1e30), (1e-9, 1e30, 0.0, 0.0)]
    for row in rows:
        if bound_passes(*row):
            passed += 1
            assert extreme_u(*row) < TWO20, row
        else:
            refused += 1
    assert bound_passes(0.2, 0.2, 0.1, 0.1) and bound_passes(0.2, 0.3, 0.1, 1.0) and bound_passes(1e30, 1e30, 0.0, 0.0)
    assert not bound_passes(1e-6, 1e-6, 1.0, 0.1) and not bound_passes(1e-9, 1e30, 0.0, 0.0)
    assert passed > 1000 and refused > 100, (passed, refused)
