"""Integer and digit-level models of GA's N-adic joint tail (csrc/modexp.hip
modexp_nadic_tail_kernel): the tail of s^E * c^-e mod N^2 in the head's pair form.
Pure Python, no GPU.

The tail takes the head's raw pair and its 64 odd powers, enters base2 = c^-1 =
lo + 2^2048 hi in ONE coupled pass with both halves streamed,
    A: (t, M) = red(lo r + hi r2)      B: h = red(lo nq + hi nq2 + M)
(M(R) = (r, nq) the pair of R^2, P2 = (r2, nq2) the pair of 2^2048 R^2), builds
T2[u] = T2[u-1] T2[1] from T2[0] = (1, 0) M(R), runs the bits below 256 with the
head's squaring, the head's sliding windows carried on over the low bits and a
product by T2[nibble of e] every fourth bit, and leaves through the full-width
hand-over of test_nadic_model.handover."""
import math
import random

from test_nadic_model import (D, KH, L, LO, MASK, RF, RH, entry_const, handover, head, lazy, nmul, nsqr, red, scaled,
                              to_digits, undigits, value)
from test_nadic_onepass_model import A_MAX, product_pair2

W = 7
SPLIT = 2048


def p2_const(Np):
    """P2: 2^2048 R^2 mod N'^2 split by N' like M(R)"""
    q, r = divmod((RH * RH << SPLIT) % (Np * Np), Np)
    return r, (Np - q) % Np


def enter2(c, Np):
    """the pair of c R from c < 2^4096, one pass: no pairs are added"""
    lo, hi = c & ((1 << SPLIT) - 1), c >> SPLIT
    MR, P2 = entry_const(Np), p2_const(Np)
    t, M = red(lo * MR[0] + hi * P2[0], Np)
    h, _ = red(lo * MR[1] + hi * P2[1] + M, Np)
    return t, h


def odd_powers(s, N):
    """the table the head leaves behind, whatever its exponent"""
    Np = scaled(N)
    x = nmul((s, 0), entry_const(Np), Np)
    x2 = nsqr(x, Np)
    T = [x]
    for _ in range(1, 1 << (W - 1)):
        T.append(nmul(T[-1], x2, Np))
    return T


def tail(x, T, s, E, cinv, e, N, check):
    """the tail's loop and exit; returns (result mod N^2, loop products)"""
    Np = scaled(N)
    NN = N * N
    T2 = [nmul((1, 0), entry_const(Np), Np), enter2(cinv, Np)]
    for _ in range(2, 16):
        T2.append(nmul(T2[-1], T2[1], Np))
    for u, row in enumerate(T2):
        check(row, Np)
        assert value(row, Np) % NN == pow(cinv, u, NN) * RH % NN
    products = 0
    pend_at, pend_d = -1, 0
    for i in range(LO - 1, -1, -1):
        if pend_at < 0 and (E >> i) & 1:
            j = max(i - W + 1, 0)
            while not (E >> j) & 1:
                j += 1
            pend_at, pend_d = j, (E >> j) & ((1 << (i - j + 1)) - 1)
        x = nsqr(x, Np)
        check(x, Np)
        if i == pend_at:
            x = nmul(x, T[pend_d >> 1], Np)
            check(x, Np)
            products += 1
            pend_at = -1
        if i & 3 == 0:
            x = nmul(x, T2[(e >> i) & 15], Np)
            check(x, Np)
            products += 1
    Y = handover(x, N, Np)
    return Y * pow(RF, -1, NN) % NN, products


def run(s, E, cinv, e, N):
    worst = [0.0]

    def check(x, Np):
        assert max(x) < Np + Np // 64 + 2
        worst[0] = max(worst[0], max(x) / Np)

    x, Np = head(s, E, N, w=W, check=check)
    got, products = tail(x, odd_powers(s, N), s, E, cinv, e, N, check)
    NN = N * N
    assert got == pow(s, E, NN) * pow(cinv, e, NN) % NN
    return worst[0], products


def moduli():
    rng = random.Random(21)
    return [rng.getrandbits(2048) | (1 << 2047) | 1, rng.getrandbits(2047) | (1 << 2046) | 1,
            rng.getrandbits(1500) | (1 << 1499) | 1, 2 ** 2048 - 1, 3]


def test_p2_split():
    for N in moduli():
        Np = scaled(N)
        r2, nq2 = p2_const(Np)
        assert 0 <= r2 < Np and 0 <= nq2 < Np
        assert (r2 - nq2 * Np) % (Np * Np) == (RH * RH << SPLIT) % (Np * Np)


def test_one_pass_entry():
    """the pair of c R for every c < 2^4096, within the chain's bound"""
    rng = random.Random(22)
    for N in moduli():
        Np = scaled(N)
        NN = N * N
        for c in (0, 1, NN - 1, 2 ** 2048 - 1, 2 ** 2048, 2 ** 4096 - 1, rng.randrange(NN), rng.getrandbits(4096)):
            x = enter2(c, Np)
            assert value(x, Np) == c * RH % (Np * Np)
            assert value(x, Np) % NN == c * RH % NN
            assert max(x) < Np + Np // 64 + 2


def test_whole_tail():
    """22 chains: every modulus with edge and random operands, exponents shorter than
    the split and with bits on both sides of bit 256"""
    rng = random.Random(23)
    chains = 0
    for N in moduli():
        NN = N * N
        s = rng.getrandbits(2048)
        cases = [(N, rng.randrange(NN), rng.getrandbits(256)),
                 (N, NN - 1, 2 ** 256 - 1),
                 (N, 1, 0),
                 ((0x5B << 252) | rng.getrandbits(200), rng.randrange(NN), 1),      # a window's bits on both sides of bit 256
                 (rng.getrandbits(200) | 1, NN - 1, rng.getrandbits(256))]        # shorter than the split
        if N == 3:
            cases = [(3, 8, 2 ** 256 - 1), (rng.getrandbits(300) | (1 << 299), 1, 5), (0, 7, 0)]
        if N == 2 ** 2048 - 1:
            cases = cases[:4]
        for E, cinv, e in cases:
            worst, products = run(s, E, cinv, e, N)
            assert worst <= 1.0001
            assert 64 <= products <= 64 + 256 // (W + 1) + 8
            if E.bit_length() > 2000:
                assert 90 <= products <= 104
            chains += 1
    assert chains == 22


def test_two_operand_rows_with_a_side_second_operand():
    """the entry's pass: both register operands non-zero in group A too; digits of the
    constants are exact (< 2^29), the streamed halves of c are exact digits"""
    rng = random.Random(24)
    for N in moduli():
        Np = scaled(N)
        n = to_digits(Np)
        MR, P2 = entry_const(Np), p2_const(Np)
        for c in (rng.getrandbits(4096), 2 ** 4096 - 1, 2 ** 2048, 1):
            lo, hi = c & ((1 << SPLIT) - 1), c >> SPLIT
            oA, oB, peak = product_pair2(to_digits(lo), to_digits(hi), to_digits(MR[0]), to_digits(MR[1]),
                                         to_digits(P2[0]), to_digits(P2[1]), n)
            assert (undigits(oA), undigits(oB)) == enter2(c, Np)
            assert peak < 1 << 64
        # lazy operands on every side (the rows do not care which side is a constant)
        top = Np + Np // 64 + 1
        for _ in range(2):
            a, a2, bA, bB, b2A, b2B = (rng.randrange(top) for _ in range(6))
            oA, oB, peak = product_pair2(lazy(a, rng, 127), lazy(a2, rng, 127), lazy(bA, rng, 127), lazy(bB, rng, 127),
                                         lazy(b2A, rng, 127), lazy(b2B, rng, 127), n)
            t, M = red(a * bA + a2 * b2A, Np)
            h, _ = red(a * bB + a2 * b2B + M, Np)
            assert (undigits(oA), undigits(oB)) == (t, h)
            assert peak < 1 << 64


def test_column_bound_a_side_second_operand():
    """all-maximal digits in both groups and both operands: the peak column stays
    below 2^64 (group A's stay collects what group B's does, less the coupling digit)"""
    a = [A_MAX] * KH
    n = [MASK] * KH
    _, _, peak = product_pair2(a, a, a, a, a, a, n, bounded=False)
    assert peak < 1 << 64
    col = 2 * L * A_MAX * A_MAX + L * MASK * MASK + MASK + (1 << 35) + (1 << D)
    assert peak <= col and math.log2(col) < 62.8
