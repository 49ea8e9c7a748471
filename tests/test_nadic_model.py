"""Integer and digit-level models of the half-width N-adic Montgomery product
that GA's s^N mod N^2 head runs (csrc/mont29.hpp product_pair, csrc/modexp.hip
modexp_nadic_head_kernel).  Pure Python, no GPU.

A residue X mod N'^2 (N' = N k0, k0 = -N^-1 mod 2^29, so N' = -1 mod 2^29) is the
pair (x0, x1) with X = x0 - x1 N'.  With red(T) = (t, M), T + M N' = t R exactly
(R = 2^(29*72)), the product of (a0, a1) and (b0, b1) is
    (t, M) = red(a0 b0),  (h, .) = red(a0 b1 + a1 b0 + M)
and (t, h) represents X(a) X(b) / R mod N'^2.  The tests check that model against
pow(), the entry constant M(R), the hand-over to the full-width chain
(Y = x0 C1 + x1 C2 / R_full), and the 64-bit column bound of the coupled rows."""
import math
import random

import pytest

D = 29
KH = 72                  # digits of the half width
RH = 1 << (D * KH)       # R of the half-width rows
RF = RH * RH             # R of the full-width (144-digit) chain the tail runs
L, G = 9, 8
MASK = (1 << D) - 1
LO = 256                 # the head runs the exponent bits >= LO


def scaled(N):
    k0 = (-pow(N, -1, 1 << D)) % (1 << D)
    return N * k0


def red(T, Np):
    """the row loop: 72 quotient digits, each the retiring digit itself"""
    M = 0
    for i in range(KH):
        m = T & MASK
        M |= m << (D * i)
        T = (T + m * Np) >> D
    return T, M


def nmul(a, b, Np):
    t, M = red(a[0] * b[0], Np)
    h, _ = red(a[0] * b[1] + a[1] * b[0] + M, Np)
    return t, h


def nsqr(a, Np):
    t, M = red(a[0] * a[0], Np)
    h, _ = red(a[0] * (2 * a[1]) + M, Np)
    return t, h


def value(x, Np):
    return (x[0] - x[1] * Np) % (Np * Np)


def entry_const(Np):
    """M(R): R^2 mod N'^2 split by N' as (r, (N' - q) mod N')"""
    q, r = divmod(RH * RH % (Np * Np), Np)
    return r, (Np - q) % Np


def head(s, E, N, w=7, check=None):
    """x = s^(E >> LO) in N-adic Montgomery form, by the head's sliding windows"""
    Np = scaled(N)
    MR = entry_const(Np)
    top = E.bit_length() - 1
    if top < LO:
        return nmul((1, 0), MR, Np), Np
    x = nmul((s, 0), MR, Np)
    assert value(x, Np) == s * RH % (Np * Np)
    x2 = nsqr(x, Np)
    tw = 1 << (w - 1)
    T = [x]
    for _ in range(1, tw):
        T.append(nmul(T[-1], x2, Np))
    acc, i, first = None, top, True
    while i >= LO:
        if not (E >> i) & 1:
            acc = nsqr(acc, Np)
            i -= 1
            continue
        j = max(i - w + 1, LO)
        while not (E >> j) & 1:
            j += 1
        d = (E >> j) & ((1 << (i - j + 1)) - 1)
        if first:
            acc, first = T[d >> 1], False
        else:
            for _ in range(i - j + 1):
                acc = nsqr(acc, Np)
                if check:
                    check(acc, Np)
            acc = nmul(acc, T[d >> 1], Np)
        if check:
            check(acc, Np)
        i = j - 1
    return acc, Np


def handover(x, N, Np):
    """the tail's entry: Y = x R_full mod N^2 in the full-width chain, from the raw
    pair: Y = mont(x0, C1) + mont(x1, C2) with C1 = R^3, C2 = -N' R^3 mod N^2
    (mont = the full-width product modulo (N^2)' = N^2 k, k = -N^-2 mod 2^29)"""
    NN = N * N
    NNp = scaled(NN)
    C1 = RH * RF % NN
    C2 = (NN - Np % NN) * C1 % NN

    def mont(a, b):
        T = a * b
        for _ in range(2 * KH):
            T = (T + (T & MASK) * NNp) >> D
        return T

    Y = mont(x[0], C1) + mont(x[1], C2)
    assert Y < 2 * NNp
    return Y


def run_chain(s, E, N):
    bounds = []

    def check(x, Np):
        bounds.append(max(x) / Np)

    x, Np = head(s, E, N, check=check)
    NN = N * N
    want = pow(s, E >> LO, NN)
    assert value(x, Np) % NN == want * RH % NN
    # exit as the issue writes it: strip R, X = x0 + (2N' - x1) N'
    e = nmul(x, (1, 0), Np)
    assert (e[0] + (2 * Np - e[1]) * Np) % NN == want
    # the hand-over the kernels use, then the remaining bits as plain arithmetic
    Y = handover(x, N, Np)
    assert Y % NN == want * RF % NN
    rest = Y * pow(RF, -1, NN) % NN
    got = pow(rest, 1 << LO, NN) * pow(s, E & ((1 << LO) - 1), NN) % NN
    assert got == pow(s, E, NN)
    return max(bounds) if bounds else 1.0


def test_integer_model_random():
    rng = random.Random(7)
    for bits in (2048, 2048, 2047, 1500):
        N = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        s = rng.getrandbits(2048)
        worst = run_chain(s, N, N)
        assert worst <= 2.02     # x1 after a table product is a sum of two outputs
    for N, s in ((3, 2), (3, 2 ** 2048 - 1)):
        run_chain(s, N, N)
        run_chain(s, rng.getrandbits(300) | (1 << 299), N)


def test_integer_model_all_ones():
    N = 2 ** 2048 - 1
    run_chain(2 ** 2048 - 1, N, N)
    run_chain(N - 1, N, N)
    run_chain(0, N, N)
    run_chain(1, N, N)
    run_chain(5, 0, N)
    run_chain(5, (1 << 200) + 12345, N)


def test_entry_split():
    rng = random.Random(11)
    for N in (2 ** 2048 - 1, 3, rng.getrandbits(2048) | (1 << 2047) | 1):
        Np = scaled(N)
        assert Np & MASK == MASK and Np < 1 << 2077 and RH // Np >= 1 << 11
        r, nq = entry_const(Np)
        assert 0 <= r < Np and 0 <= nq < Np
        assert (r - nq * Np) % (Np * Np) == RH * RH % (Np * Np)


# ---- digit-level model of the coupled rows -------------------------------------
# 16 lanes: group A (lanes 0-7) and group B (lanes 8-15), L = 9 lazy 64-bit columns
# each; both stream the same 72 digits; lane 8 adds group A's quotient digit to its
# retiring column before group B's own quotient digit is taken.

def to_digits(v, n=KH):
    return [(v >> (D * i)) & MASK for i in range(n)]


def lazy(v, rng, extra):
    """digits of v in the lazy form a finished product leaves (<= 2^29 + extra):
    borrow from the digit above where that keeps every digit in range"""
    d = to_digits(v)
    for i in range(KH - 1):
        if d[i + 1] > 0 and d[i] <= extra - 1 and rng.random() < 0.5:
            d[i] += 1 << D
            d[i + 1] -= 1
    return d


def product_pair(a, bA, bB, n, coupled, bounded=True):
    """digits in, lazy digits out; returns (outA, outB, max column seen)"""
    acc = [[0] * L for _ in range(16)]
    b = [bA[g * L:(g + 1) * L] for g in range(G)] + [bB[g * L:(g + 1) * L] for g in range(G)]
    nd = [n[(g % G) * L:(g % G + 1) * L] for g in range(16)]
    peak = 0
    for r in range(KH):
        R = r % L
        s0, s1 = R % L, (R + 1) % L
        for ln in range(16):
            for j in range(L):
                acc[ln][(j + R) % L] += a[r] * b[ln][j]
        mA = acc[0][s0] & MASK
        if coupled:
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
        assert not bounded or max(cols) <= (1 << D) + 127
        return cols
    return finish(range(8)), finish(range(8, 16)), peak


def undigits(d):
    return sum(c << (D * i) for i, c in enumerate(d))


def test_coupled_rows_match_integer_model():
    rng = random.Random(3)
    for N in (rng.getrandbits(2048) | (1 << 2047) | 1, 2 ** 2048 - 1):
        Np = scaled(N)
        n = to_digits(Np)
        a = (rng.randrange(Np), rng.randrange(2 * Np))
        y = (rng.randrange(Np), rng.randrange(2 * Np))
        # squaring: A's operand x0, B's 2 x1 (digits doubled, as the kernel does)
        a0 = lazy(a[0], rng, 127)
        a1 = lazy(a[1], rng, 254)
        oA, oB, peak = product_pair(a0, a0, [2 * v for v in a1], n, True)
        assert (undigits(oA), undigits(oB)) == nsqr(a, Np)
        assert peak < 1 << 64
        # table product: pass alpha streams y0 (A: x0, B: x1, coupled), pass beta
        # streams the old x0 (B: y1, uncoupled), x1 = h_alpha + h_beta
        y0, y1 = lazy(y[0], rng, 127), lazy(y[1], rng, 254)
        tA, hA, p1 = product_pair(y0, a0, a1, n, True)
        _, hB, p2 = product_pair(a0, a0, y1, n, False)
        t, h = nmul(a, y, Np)
        assert undigits(tA) == t
        assert (undigits(hA) + undigits(hB) - h) % Np == 0
        got = (undigits(tA), undigits(hA) + undigits(hB))
        assert value(got, Np) == value(a, Np) * value(y, Np) * pow(RH, -1, Np * Np) % (Np * Np)
        assert max(p1, p2) < 1 << 64


def stay_weights_pair():
    """products a column of the coupled rows collects during its L-row stay in one
    lane: one a*b and one m*n per row (every row is a plain row), as
    test_column_bound.stay_weights enumerates them"""
    ab, mn = {}, {}
    for r in range(KH):
        for g in range(G):
            for j in range(L):
                key = (r + g * L + j, g)
                ab[key] = ab.get(key, 0) + 1
                mn[key] = mn.get(key, 0) + 1
    return max(ab.values()), max(mn.values())


def test_column_bound_pair():
    """worst case of a stay: the streamed digit <= 2^29 + 127 (a finished product),
    the register digit <= 2 (2 (2^29 + 127)) = 2^31 + 508 (x1 summed over the two
    passes of a table product, then doubled for a squaring), one m*n < 2^58 per
    row, the quotient digit of group A (< 2^29) once, the carry of the column
    retired before it (< 2^35) and the digit moved down (< 2^29)"""
    ab, mn = stay_weights_pair()
    assert ab == L and mn == L
    a_max = (1 << D) + 127
    b_max = 4 * a_max
    col = ab * a_max * b_max + mn * MASK * MASK + MASK + (1 << 35) + (1 << D)
    assert math.log2(col) < 63.6
    assert col < 1 << 64


def test_column_bound_pair_adversarial():
    """all-maximal digits through the digit model: the peak column stays < 2^64"""
    a = [(1 << D) + 127] * KH
    bB = [4 * ((1 << D) + 127)] * KH
    n = [MASK] * KH
    _, _, peak = product_pair(a, a, bB, n, True, bounded=False)   # operands past R: only the columns matter
    assert peak < 1 << 64
