"""Digit-level model of the one-pass N-adic table product (csrc/mont29.hpp
product_pair2, csrc/modexp.hip modexp_nadic_head_kernel).  Pure Python, no GPU.

A table product (x0, x1) (y0, y1) / R streams TWO operands through the same 72
coupled rows, y0 and the old x0, each with its own register operand:
    A: acc += y0_i x0 + x0_i 0          B: acc += y0_i x1 + x0_i y1
so the pass computes (t, M) = red(x0 y0) in A and h = red(x0 y1 + x1 y0 + M) in B:
test_nadic_model.nmul itself, one reduction, instead of red(T1) + red(T2) (which
agrees with it only mod N').  x1 is then a single finished product, so the operand
a squaring doubles has digits <= 2 (2^29 + 127)."""
import math
import random

from test_nadic_model import (D, G, KH, L, MASK, RH, entry_const, lazy, nmul, nsqr, scaled, to_digits,
                              undigits, value)

A_MAX = (1 << D) + 127   # digit of a finished product


def product_pair2(a, a2, bA, bB, b2A, b2B, n, bounded=True):
    """the coupled rows with two streamed operands: digits in, lazy digits out;
    returns (outA, outB, max column seen)"""
    acc = [[0] * L for _ in range(16)]

    def split(vA, vB):
        return [vA[g * L:(g + 1) * L] for g in range(G)] + [vB[g * L:(g + 1) * L] for g in range(G)]

    b, b2 = split(bA, bB), split(b2A, b2B)
    nd = [n[(g % G) * L:(g % G + 1) * L] for g in range(16)]
    peak = 0
    for r in range(KH):
        R = r % L
        s0, s1 = R % L, (R + 1) % L
        for ln in range(16):
            for j in range(L):
                acc[ln][(j + R) % L] += a[r] * b[ln][j] + a2[r] * b2[ln][j]
        mA = acc[0][s0] & MASK
        acc[8][s0] += mA
        mB = acc[8][s0] & MASK
        for ln in range(16):
            m = mA if ln < 8 else mB
            for j in range(L):
                acc[ln][(j + R) % L] += m * nd[ln][j]
        peak = max(peak, max(max(c) for c in acc))
        moved = []
        for ln in range(16):
            acc[ln][s1] += acc[ln][s0] >> D
            moved.append(acc[ln][s0] & MASK)
        assert moved[0] == 0 and moved[8] == 0
        for ln in range(16):
            acc[ln][s0] = 0 if ln % G == G - 1 else moved[ln + 1]
        peak = max(peak, max(max(c) for c in acc))

    def finish(lanes):
        cols = [c for ln in lanes for c in acc[ln]]   # rotation is back to identity
        v = sum(c << (D * i) for i, c in enumerate(cols))
        for _ in range(2):                            # two parallel carry steps
            cols = [(cols[i] & MASK) + (cols[i - 1] >> D if i else 0) for i in range(KH)]
        assert not bounded or sum(c << (D * i) for i, c in enumerate(cols)) == v
        assert not bounded or max(cols) <= A_MAX
        return cols
    return finish(range(8)), finish(range(8, 16)), peak


def test_two_operand_rows_match_nmul():
    """the pass is nmul exactly (not only mod N'), for random and edge operands"""
    rng = random.Random(5)
    zero = [0] * KH
    for N in (rng.getrandbits(2048) | (1 << 2047) | 1, 2 ** 2048 - 1, rng.getrandbits(1500) | (1 << 1499) | 1, 3):
        Np = scaled(N)
        n = to_digits(Np)
        top = Np + Np // 64 + 1   # the bound on x0 and x1
        cases = [((rng.randrange(top), rng.randrange(top)), (rng.randrange(top), rng.randrange(top))) for _ in range(2)]
        cases += [((top, top), (top, top)), ((0, 0), (top, top)), ((1, 0), (0, top)), ((top, 0), (top, 0))]
        for x, y in cases:
            x0, x1 = lazy(x[0], rng, 127), lazy(x[1], rng, 127)
            y0, y1 = lazy(y[0], rng, 127), lazy(y[1], rng, 127)
            oA, oB, peak = product_pair2(y0, x0, x0, x1, zero, y1, n)
            assert (undigits(oA), undigits(oB)) == nmul(x, y, Np)
            assert peak < 1 << 64


def test_chain_bounds_one_pass():
    """the head's schedule with every table product a single nmul: the value is
    s^(E >> LO) R mod N'^2 and x0, x1 stay below N' (1 + 2^-6) + 2, so a doubled x1
    has digits <= 2 (2^29 + 127) once normalised"""
    rng = random.Random(9)
    for bits in (2048, 2047, 1500, 2):
        N = 3 if bits == 2 else rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        Np = scaled(N)
        lim = Np + Np // 64 + 2
        s = rng.getrandbits(2048)
        x = nmul((s, 0), entry_const(Np), Np)
        assert max(x) < lim
        x2 = nsqr(x, Np)
        T = [x]
        for _ in range(1, 64):
            T.append(nmul(T[-1], x2, Np))
            assert max(T[-1]) < lim
        acc, e = T[-1], 127
        for _ in range(40):
            for _ in range(rng.randrange(1, 9)):
                acc = nsqr(acc, Np)
                e *= 2
                assert max(acc) < lim
            k = rng.randrange(64)
            acc = nmul(acc, T[k], Np)
            e += 2 * k + 1
            assert max(acc) < lim
        assert value(acc, Np) == pow(s, e, Np * Np) * RH % (Np * Np)


def stay_weights_two():
    """products a column collects during its L-row stay in one lane: two a*b and
    one m*n per row (test_nadic_model.stay_weights_pair with the second operand)"""
    ab, mn = {}, {}
    for r in range(KH):
        for g in range(G):
            for j in range(L):
                key = (r + g * L + j, g)
                ab[key] = ab.get(key, 0) + 2
                mn[key] = mn.get(key, 0) + 1
    return max(ab.values()), max(mn.values())


def test_column_bound_two_operands():
    """worst case of a stay: streamed and register digits <= 2^29 + 127 (finished
    products: x1 is no longer a sum), one m*n < 2^58 per row, group A's quotient
    digit (< 2^29) once, the carry of the column retired before it (< 2^35) and
    the digit moved down (< 2^29)"""
    ab, mn = stay_weights_two()
    assert ab == 2 * L and mn == L
    col = ab * A_MAX * A_MAX + mn * MASK * MASK + MASK + (1 << 35) + (1 << D)
    assert math.log2(col) < 62.8
    assert col < 1 << 64


def test_column_bound_squaring_after_one_pass():
    """the squaring's doubled operand shrinks to 2 (2^29 + 127)"""
    col = L * A_MAX * 2 * A_MAX + L * MASK * MASK + MASK + (1 << 35) + (1 << D)
    assert math.log2(col) < 62.8


def test_column_bound_two_operands_adversarial():
    """all-maximal digits through the digit model: the peak column stays < 2^64"""
    a = [A_MAX] * KH
    n = [MASK] * KH
    _, _, peak = product_pair2(a, a, a, a, a, a, n, bounded=False)   # operands past R: only the columns matter
    assert peak < 1 << 64
    assert math.log2(peak) < 62.8
