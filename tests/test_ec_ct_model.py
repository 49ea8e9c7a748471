"""A Python model of exactly what the secret-scalar secp256k1 kernels compute
(csrc/secp256k1_ct.hpp, csrc/ec_ct.hip), against the oracle's curve arithmetic
(oracle/secp256k1.py):

  * the complete projective addition, mixed addition and doubling, in the
    header's product schedule, over every pair from {O, G, -G, random points}
    with random projective scalings;
  * the nibble comb k G = sum_i T[i][k_i] - C with the +1 offset, as one sum and
    as the kernel's four groups of 16 windows combined by two rounds of sums;
  * the variable-base window loop (four doublings, one table addition per
    nibble from the top) for P = G, -G and O;
  * the masked field reductions at limb level (32-bit limbs, 64-bit carries,
    wrap-around as on the device).

The model is imported by the GPU tests for the edge scalar list."""
import os
import random
import re

from oracle import secp256k1 as ec

from test_ec_glv import EDGE

P, N = ec.P, ec.Q
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
ID = (0, 1, 0)
C_SCALAR = (16 ** 64 - 1) // 15
# the scalars at which the comb's running sum meets C, -C or the identity, the
# ends of the range (no reduction mod q on the device) and the nibble extremes
EDGE_CT = [k % 2 ** 256 for k in EDGE] + [N, N + 1, 2 ** 256 - 1, C_SCALAR % N, (-C_SCALAR) % N, C_SCALAR,
                                          2 ** 256 - N, 2 ** 256 - 2]
EDGE_CT = list(dict.fromkeys(EDGE_CT))   # 0 and 2^256 - 1 (every nibble 0 / 15) appear once


# ------------------------------------------------------------ group law model ----
def padd(p, q):
    """proj_add_ct: 12 products."""
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    xx, yy, zz0 = X1 * X2 % P, Y1 * Y2 % P, Z1 * Z2 % P
    s = ((X1 + Y1) * (X2 + Y2) - xx - yy) % P
    u = ((Y1 + Z1) * (Y2 + Z2) - yy - zz0) % P
    w = ((X1 + Z1) * (X2 + Z2) - xx - zz0) % P
    return _tail(xx, yy, zz0, s, u, w)


def padd_aff(p, a):
    """proj_add_aff_ct: p + (x2 : y2 : 1), 11 products."""
    X1, Y1, Z1 = p
    x2, y2 = a
    xx, yy = X1 * x2 % P, Y1 * y2 % P
    s = ((X1 + Y1) * (x2 + y2) - xx - yy) % P
    u = (y2 * Z1 + Y1) % P
    w = (x2 * Z1 + X1) % P
    return _tail(xx, yy, Z1, s, u, w)


def _tail(xx, yy, zz0, s, u, w):
    zz, xx3, w21 = 21 * zz0 % P, 3 * xx % P, 21 * w % P
    d, e = (yy - zz) % P, (yy + zz) % P
    return ((s * d - u * w21) % P, (e * d + xx3 * w21) % P, (u * e + xx3 * s) % P)


def pdbl(p):
    """proj_dbl_ct: 8 products."""
    X, Y, Z = p
    t, z = Y * Y % P, 21 * Z * Z % P
    d, e = (t - 3 * z) % P, (t + z) % P
    return (2 * X * Y * d % P, (d * e + 8 * t * z) % P, 8 * t * Y * Z % P)


def to_aff(p):
    """proj_to_aff_ct: Fermat inverse maps Z = 0 to 0, so the identity gives (0, 0) = None."""
    X, Y, Z = p
    zi = pow(Z, P - 2, P)
    x, y = X * zi % P, Y * zi % P
    return None if (x, y) == (0, 0) else (x, y)


def from_aff(pt):
    """proj_from_aff_ct: the ABI's (0, 0) becomes (0 : 1 : 0)."""
    return ID if pt is None else (pt[0], pt[1], 1)


def _points(rnd, count):
    return [None, ec.G, ec.neg(ec.G)] + [ec.mul(ec.G, rnd.randrange(1, N)) for _ in range(count)]


def _scaled(rnd, pt):
    X, Y, Z = from_aff(pt)
    lam = rnd.randrange(1, P)
    return (X * lam % P, Y * lam % P, Z * lam % P)


def test_complete_addition_all_pairs():
    rnd = random.Random(21)
    pts = _points(rnd, 6)
    for a in pts:
        for b in pts:
            assert to_aff(padd(_scaled(rnd, a), _scaled(rnd, b))) == ec.add(a, b)
            if b is not None:
                assert to_aff(padd_aff(_scaled(rnd, a), b)) == ec.add(a, b)


def test_complete_doubling():
    rnd = random.Random(22)
    for a in _points(rnd, 8):
        assert to_aff(pdbl(_scaled(rnd, a))) == ec.add(a, a)


# ------------------------------------------------------------------ the comb ----
_TABLE = None


def comb_table():
    """T[i][d] = (d + 1) 16^i G (affine) and -C, as ec_ct_host.cpp builds them."""
    global _TABLE
    if _TABLE is None:
        rows, B, C = [], ec.G, None
        for _ in range(64):
            C = ec.add(C, B)
            row, T = [], B
            for d in range(16):
                row.append(T)
                T = ec.add(T, B)
            rows.append(row)
            B = row[15]
        _TABLE = (rows, ec.neg(C))
    return _TABLE


def comb(k, groups=1):
    """ec_mul_g_ct_kernel: `groups` partial sums over consecutive windows, each
    from the identity by mixed additions, combined pairwise, then -C."""
    rows, negC = comb_table()
    per = 64 // groups
    part = []
    for j in range(groups):
        acc = ID
        for i in range(per * j, per * (j + 1)):
            acc = padd_aff(acc, rows[i][(k >> (4 * i)) & 15])
        part.append(acc)
    while len(part) > 1:   # the __shfl_xor rounds: (0,1) and (2,3), then the halves
        part = [padd(part[i], part[i + 1]) for i in range(0, len(part), 2)]
    return to_aff(padd_aff(part[0], negC))


def test_comb_table_has_no_identity():
    rows, negC = comb_table()
    assert all(pt is not None and ec.is_on_curve(pt) for row in rows for pt in row)
    assert negC == ec.neg(ec.mul(ec.G, C_SCALAR % N)) and negC is not None
    assert rows[63][15] == ec.mul(ec.G, 16 ** 64 % N) and rows[5][2] == ec.mul(ec.G, 3 * 16 ** 5)


def test_comb_edge_and_random_scalars():
    rnd = random.Random(23)
    assert 0 in EDGE_CT and 2 ** 256 - 1 in EDGE_CT and N - 1 in EDGE_CT and N + 1 in EDGE_CT
    for k in EDGE_CT + [rnd.randrange(2 ** 256) for _ in range(8)]:
        assert comb(k) == ec.mul(ec.G, k % N), hex(k)


def test_comb_in_four_groups():
    rnd = random.Random(24)
    for k in EDGE_CT + [rnd.randrange(2 ** 256) for _ in range(8)]:
        assert comb(k, groups=4) == ec.mul(ec.G, k % N), hex(k)


# ------------------------------------------------------ variable-base windows ----
def window_mul(pt, k):
    """ec_msm_ct_term_kernel: table d P (d = 0 the identity), 64 windows from the top."""
    T = [ID, from_aff(pt)]
    for d in range(2, 16):
        T.append(padd(T[d - 1], T[1]))
    acc = ID
    for w in range(63, -1, -1):
        for _ in range(4):
            acc = pdbl(acc)
        acc = padd(acc, T[(k >> (4 * w)) & 15])
    return acc


def test_variable_base_windows():
    rnd = random.Random(25)
    for pt in (ec.G, ec.neg(ec.G), None):
        for k in EDGE_CT[:6] + [N, 2 ** 256 - 1, rnd.randrange(2 ** 256)]:
            assert to_aff(window_mul(pt, k)) == ec.mul(pt, k % N)
    k = rnd.randrange(1, N)
    pt = ec.mul(ec.G, 77)
    assert to_aff(padd(window_mul(pt, k), window_mul(pt, N - k))) is None   # ec_msm_ct_sum: an identity output


# ------------------------------------------------- limb-level field reductions ----
def limbs(x):
    return [(x >> (32 * i)) & M32 for i in range(8)]


def value(v):
    return sum(x << (32 * i) for i, x in enumerate(v))


PL = limbs(P)


def fe_tail(r, cc):
    """fe_tail_ct: r + cc 2^256 (< 2p) fully reduced through one masked selection."""
    t, c = [0] * 8, r[0] + 977
    t[0] = c & M32
    c = (c >> 32) + r[1] + 1
    t[1] = c & M32
    c >>= 32
    for i in range(2, 8):
        c += r[i]
        t[i] = c & M32
        c >>= 32
    m = (0 - (cc | c)) & M32
    return [(t[i] & m) | (r[i] & ~m & M32) for i in range(8)]


def fe_add(a, b):
    s, c = [0] * 8, 0
    for i in range(8):
        c += a[i] + b[i]
        s[i] = c & M32
        c >>= 32
    return fe_tail(s, c)


def fe_sub(a, b):
    t, br = [0] * 8, 0
    for i in range(8):
        d = a[i] - b[i] + br
        t[i] = d & M32
        br = d >> 32          # 0 or -1, as the device's arithmetic shift
    m = br & M32
    r, c = [0] * 8, 0
    for i in range(8):
        c += t[i] + (PL[i] & m)
        r[i] = c & M32
        c >>= 32
    return r


def fe_mul_small(a, k):
    s, c = [0] * 8, 0
    for i in range(8):
        c += a[i] * k
        s[i] = c & M32
        c >>= 32
    h = c
    c = s[0] + h * 977
    s[0] = c & M32
    c = (c >> 32) + s[1] + h
    s[1] = c & M32
    c >>= 32
    for i in range(2, 8):
        c += s[i]
        s[i] = c & M32
        c >>= 32
    return fe_tail(s, c)


def fe_mul(a, b):
    t, acc = [0] * 16, 0
    for col in range(15):
        for i in range(8):
            j = col - i
            if 0 <= j <= 7:
                acc += a[i] * b[j]
        assert acc < 1 << 96                      # the 96-bit column accumulator
        t[col] = acc & M32
        acc >>= 32
    t[15] = acc & M32
    u, c = [0] * 10, 0
    for i in range(10):
        s = c
        if i < 8:
            s += t[i] + t[8 + i] * 977
        if 1 <= i <= 8:
            s += t[8 + i - 1]
        assert s <= M64
        u[i] = s & M32
        c = s >> 32
    h = (u[9] << 32) | u[8]
    assert h < 1 << 34
    r = [0] * 8
    s0 = u[0] + (h & M32) * 977
    r[0] = s0 & M32
    s1 = (s0 >> 32) + u[1] + (h >> 32) * 977 + (h & M32)
    r[1] = s1 & M32
    s2 = (s1 >> 32) + u[2] + (h >> 32)
    r[2] = s2 & M32
    cc = s2 >> 32
    for i in range(3, 8):
        cc += u[i]
        r[i] = cc & M32
        cc >>= 32
    assert cc <= 1
    return fe_tail(r, cc)


FIELD_EDGE = [0, 1, P - 1, P, P + 1, 2 ** 256 - 1]


def test_masked_tail_reduction():
    for r in FIELD_EDGE + [P - 2 ** 32 - 978, 2 ** 32 + 976]:
        assert value(fe_tail(limbs(r), 0)) == r % P
        if r + 2 ** 256 < 2 * P:
            assert value(fe_tail(limbs(r), 1)) == (r + 2 ** 256) % P


def test_masked_field_operations():
    rnd = random.Random(26)
    red = [0, 1, 2, P - 1, P - 2, 2 ** 32 + 977, P - 2 ** 32 - 977, 2 ** 255] + [rnd.randrange(P) for _ in range(6)]
    for a in red:
        for b in red:
            assert value(fe_add(limbs(a), limbs(b))) == (a + b) % P
            assert value(fe_sub(limbs(a), limbs(b))) == (a - b) % P
            assert value(fe_mul(limbs(a), limbs(b))) == a * b % P
        for k in (3, 8, 21):
            assert value(fe_mul_small(limbs(a), k)) == a * k % P
    # the product's folds hold for any 256-bit operands, reduced or not
    for a in FIELD_EDGE:
        for b in FIELD_EDGE:
            assert value(fe_mul(limbs(a), limbs(b))) == a * b % P


def _table(name):
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fs-dkr_amd", "csrc",
                            "secp256k1_ct.hpp")).read()
    return [int(x) for x in re.search(name + r"\[15\] = \{([^}]*)\}", src).group(1).split(",")]


def test_fermat_inverse_chain():
    """fe_inv_ct's step tables (read from the header): 255 squarings, 15 products,
    the exponent they spell is p - 2, and 0 maps to 0."""
    nsqr, ops, keep = _table("INV_NSQR"), _table("INV_OP"), _table("INV_KEEP")
    assert sum(nsqr) == 255

    def chain(mul, sqr, a):
        kept = {0: a, 1: a, 2: a, 3: a, 4: a}     # a, x2, x3, x22, x44
        x = a
        for n, op, k in zip(nsqr, ops, keep):
            kept[5] = x
            for _ in range(n):
                x = sqr(x)
            x = mul(x, kept[op])
            if k:
                kept[k] = x
        return x
    # on exponents: squaring doubles, a product adds
    assert chain(lambda e, f: e + f, lambda e: 2 * e, 1) == P - 2
    for a in (0, 1, 2, P - 1, 0xDEADBEEF):
        assert chain(lambda u, v: u * v % P, lambda u: u * u % P, a) == (pow(a, -1, P) if a else 0)
