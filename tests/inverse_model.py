"""Lane-level model of csrc/inverse.hip coop_inverse<K32, G> and the edge inputs
the CPU and GPU inverse tests share.  Pure Python, no GPU.

The model keeps what the kernel keeps: a, b, u, v and m as NLT = G * LL radix-2^30
limbs, LL consecutive limbs per lane.  Coop::norm is modelled step by step (the
per-lane carry pass, then rounds that hand each lane's carry to the next lane, the
two-limb fast path, the r != 0 ripple), and so are shift_down, negate, the 62-bit
approximations with their nbits >= 62 clamp, the 30 inner steps and mdiv's three
outcomes.  Big integers run beside the limbs only to CHECK them:

  * every norm: sum x_j 2^(30 j) + T 2^(30 NLT) equals the value of its columns,
    every intermediate fits the kernel's int64, and no carry is pending when the
    round loop ends (the kernel's `round < G` bound rests on that);
  * every outer step: a, b are |a f + b g| / 2^30 exactly, and u, v stay in [0, m)
    with u y = a, v y = b (mod m).

inverse() returns (y^-1 mod m or None, Coverage)."""
import random

M30 = (1 << 30) - 1

SHAPES = [(64, 8), (96, 8), (96, 4), (128, 8), (192, 16), (192, 8)]   # coop_inverse<K32, G> as instantiated
COOP_G = {64: 8, 96: 8, 128: 8, 192: 16}     # inverse_coop_kernel
BATCH_G = {64: 8, 96: 4, 128: 8, 192: 8}     # inverse_batch_kernel
BATCH_KD = {64: 72, 96: 108, 128: 144, 192: 216}   # radix-2^29 digits of its Montgomery products


def shape(K32, G):
    """(LL, NLT) of CoopShape<K32, G>"""
    nlt0 = (32 * K32 + 29) // 30 + 1
    LL = (nlt0 + G - 1) // G
    return LL, LL * G


def to_limbs(x, n):
    assert 0 <= x < 1 << (30 * n)
    return [(x >> (30 * j)) & M30 for j in range(n)]


def from_limbs(x):
    x = x + [0] * (-len(x) % 4)                    # four limbs = 15 bytes
    return int.from_bytes(b"".join((x[i] | x[i + 1] << 30 | x[i + 2] << 60 | x[i + 3] << 90).to_bytes(15, "little")
                                   for i in range(0, len(x), 4)), "little")


class Coverage:
    """Which paths one or more inversions took."""
    FIELDS = ("outer_steps", "norm_calls", "neg_a", "neg_b", "mdiv_add", "mdiv_sub", "mdiv_keep", "rounds_max",
              "slow_plus", "slow_minus", "slow_top", "clamp62")

    def __init__(self, G):
        self.G = G
        self.max_rounds = 0
        for f in self.FIELDS:
            setattr(self, f, 0)

    def add(self, other):
        assert self.G == other.G
        self.max_rounds = max(self.max_rounds, other.max_rounds)
        for f in self.FIELDS:
            setattr(self, f, getattr(self, f) + getattr(other, f))

    def __repr__(self):
        return "Coverage(G=%d, max_rounds=%d, %s)" % (
            self.G, self.max_rounds, ", ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS))


class Model:
    def __init__(self, K32, G):
        self.K32, self.G = K32, G
        self.LL, self.NLT = shape(K32, G)
        assert self.LL >= 2          # norm's fast path touches limbs 0 and 1 of every lane
        self.cov = Coverage(G)

    # ---- Coop::norm: signed columns t -> limbs x in [0, 2^30) and T
    def norm(self, t, want):
        """`want`: the big-integer value the columns must have"""
        G, LL, NLT, cov = self.G, self.LL, self.NLT, self.cov
        cov.norm_calls += 1
        x = [0] * NLT
        carry = [0] * G
        for g in range(G):
            c = 0
            for j in range(g * LL, g * LL + LL):
                v = t[j] + c
                x[j] = v & M30
                c = v >> 30
            carry[g] = c
        assert max(map(abs, t)) < 1 << 62          # then every v above fits the kernel's int64
        top = carry[G - 1]
        inn = [0] + carry[:-1]                     # prev_s64: lane 0 reads 0
        assert all(abs(c) < 1 << 33 for c in inn)
        rounds = 0
        for _ in range(G):
            rounds += 1
            out = [0] * G
            for g in range(G):
                if inn[g] == 0:
                    continue                       # x unchanged, r = 0
                b = g * LL
                v = x[b] + inn[g]
                x[b] = v & M30
                r = v >> 30
                v = x[b + 1] + r
                x[b + 1] = v & M30
                r = v >> 30
                if r != 0:
                    assert r in (-1, 1)
                    if r > 0:
                        cov.slow_plus += 1
                    else:
                        cov.slow_minus += 1
                    if g == G - 1:
                        cov.slow_top += 1
                    for j in range(b + 2, b + LL):
                        v = x[j] + r
                        x[j] = v & M30
                        r = v >> 30
                out[g] = r
            top += out[G - 1]
            inn = [0] + out[:-1]
            if not any(inn):
                break
        assert not any(inn), "a carry is still pending after G rounds"
        cov.max_rounds = max(cov.max_rounds, rounds)
        if rounds == G - 1:
            cov.rounds_max += 1
        assert from_limbs(x) + (top << (30 * NLT)) == want
        return x, top

    # ---- Coop::shift_down
    def shift_down(self, x):
        assert x[0] == 0                           # "limb 0 is zero by construction"
        return x[1:] + [0]

    # ---- Coop::negate
    def negate(self, x):
        NLT = self.NLT
        assert x[NLT - 1] == 0
        t = [M30 - d for d in x]
        t[NLT - 1] = 0
        t[0] += 1
        r, T = self.norm(t, (1 << (30 * (NLT - 1))) - from_limbs(x))   # rare: once per sign fix
        assert T == 0 and r[NLT - 1] == 0
        return r

    def top32(self, x, p, o):
        NLT = self.NLT
        x0 = x[p]
        x1 = x[p + 1] if p + 1 < NLT else 0
        x2 = x[p + 2] if p + 2 < NLT else 0
        return (((x0 | (x1 << 30) | (x2 << 60)) & (2 ** 64 - 1)) >> o) & 0xFFFFFFFF

    # ---- (u f + v g) / 2^30 mod m in [0, m): limbs and value
    def mdiv(self, U, V, Mx, u, v, m, mneg_inv, f, gg):
        NLT, cov = self.NLT, self.cov
        half = 1 << (30 * (NLT - 1))
        lo = (U[0] * f + V[0] * gg) & M30
        q = (lo * mneg_inv) & M30
        w = [uu * f + vv * gg + q * mm for uu, vv, mm in zip(U, V, Mx)]
        full = u * f + v * gg + q * m
        assert full % (1 << 30) == 0 and -m < (full >> 30) < 2 * m
        out, T0 = self.norm(w, full)
        out = self.shift_down(out)
        neg = T0 < 0
        assert T0 in (0, -1) and neg == (full < 0)
        cur = (full - (T0 << (30 * NLT))) >> 30      # out's value, by norm's checked identity
        if neg:
            w = [d + mm for d, mm in zip(out, Mx)]
            w[NLT - 1] -= 1                        # the sign T0 = -1 sits at limb NLT-1 after the shift
            want = cur + m - half
        else:
            w = [d - mm for d, mm in zip(out, Mx)]
            want = cur - m
        R, T1 = self.norm(w, want)
        if neg:
            cov.mdiv_add += 1
            assert T1 == 0
            res = R
        elif T1 >= 0:
            cov.mdiv_sub += 1
            res = R
        else:
            cov.mdiv_keep += 1
            res = out
        val = want - (T1 << (30 * NLT)) if res is R else cur
        assert 0 <= val < m and ((val << 30) - (u * f + v * gg)) % m == 0
        return res, val

    # ---- coop_inverse
    def inverse(self, y, m):
        K32, NLT, cov = self.K32, self.NLT, self.cov
        assert m & 1 and 0 <= y < 1 << (32 * K32) and 0 < m < 1 << (32 * K32)
        A, B, Mx = to_limbs(y, NLT), to_limbs(m, NLT), to_limbs(m, NLT)
        U, V = to_limbs(1, NLT), to_limbs(0, NLT)
        a, b, u, v = y, m, 1, 0                    # the big integers the limbs are checked against
        m0 = m & 0xFFFFFFFF
        inv = m0
        for _ in range(5):
            inv = (inv * (2 - m0 * inv)) & 0xFFFFFFFF
        mneg_inv = (-inv) & M30
        assert (m * mneg_inv + 1) & M30 == 0
        mlen = max(j * 30 + d.bit_length() for j, d in enumerate(Mx) if d)
        assert mlen == m.bit_length()
        iters = (2 * mlen - 1 + 29) // 30
        half = 1 << (30 * (NLT - 1))

        for _ in range(iters):
            cov.outer_steps += 1
            ln = max([j * 30 + (p | q).bit_length() for j, (p, q) in enumerate(zip(A, B)) if p | q] or [0])
            assert ln == (a | b).bit_length()
            if ln < 62:
                cov.clamp62 += 1
            nbits = max(ln, 62)
            sh = nbits - 32
            p, o = sh // 30, sh % 30
            ah = (self.top32(A, p, o) << 30) | A[0]
            bh = (self.top32(B, p, o) << 30) | B[0]
            f0, g0, f1, g1 = 1, 0, 0, 1
            for _ in range(30):
                odd = ah & 1
                if odd and ah < bh:
                    ah, bh, f0, f1, g0, g1 = bh, ah, f1, f0, g1, g0
                if odd:
                    ah -= bh
                    f0 -= f1
                    g0 -= g1
                f1 *= 2
                g1 *= 2
                ah >>= 1
            assert 0 <= ah < 1 << 64 and 0 <= bh < 1 << 64
            assert max(abs(f0), abs(g0), abs(f1), abs(g1)) <= 1 << 30

            # (a, b) <- (|a f0 + b g0|, |a f1 + b g1|) / 2^30
            va = a * f0 + b * g0
            NA, T = self.norm([p * f0 + q * g0 for p, q in zip(A, B)], va)
            NA = self.shift_down(NA)
            assert T in (0, -1) and (T < 0) == (va < 0) and va % (1 << 30) == 0
            if T < 0:
                cov.neg_a += 1
                assert from_limbs(NA) == half + (va >> 30)
                NA = self.negate(NA)
                f0, g0 = -f0, -g0
            vb = a * f1 + b * g1
            NB, T = self.norm([p * f1 + q * g1 for p, q in zip(A, B)], vb)
            NB = self.shift_down(NB)
            assert T in (0, -1) and (T < 0) == (vb < 0) and vb % (1 << 30) == 0
            if T < 0:
                cov.neg_b += 1
                assert from_limbs(NB) == half + (vb >> 30)
                NB = self.negate(NB)
                f1, g1 = -f1, -g1
            A, B = NA, NB
            a, b = abs(va) >> 30, abs(vb) >> 30

            # (u, v) <- ((u f0 + v g0) / 2^30 mod m, (u f1 + v g1) / 2^30 mod m)
            NU, nu = self.mdiv(U, V, Mx, u, v, m, mneg_inv, f0, g0)
            V, v = self.mdiv(U, V, Mx, u, v, m, mneg_inv, f1, g1)
            U, u = NU, nu
            assert (u * y - a) % m == 0 and (v * y - b) % m == 0

        unit = B[0] == 1 and not any(B[1:])
        return (from_limbs(V) if unit else None), cov


def inverse(y, m, K32, G):
    """(y^-1 mod m as coop_inverse<K32, G> computes it, or None; Coverage)"""
    return Model(K32, G).inverse(y, m)


def python_inverse(y, m):
    try:
        return pow(y, -1, m)
    except ValueError:
        return None


# ------------------------------------------------------------------ edge inputs
def edge_moduli(K32):
    """[(name, m)]: the eight moduli of edge_cases"""
    rnd = random.Random(7000 + K32)
    bits = 32 * K32
    n = rnd.getrandbits(bits // 2) | 1 | (1 << (bits // 2 - 1))
    return [
        ("odd", rnd.getrandbits(bits) | 1 | (1 << (bits - 1))),
        ("nsq", n * n),
        ("short137", rnd.getrandbits(bits - 137) | 1 | (1 << (bits - 138))),
        ("ones", (1 << bits) - 1),
        ("pow2p1", (1 << (bits - 1)) + 1),
        ("halfones_sq", ((1 << (bits // 2)) - 1) ** 2),
        ("m61", rnd.getrandbits(61) | 1 | (1 << 60)),
        ("three", 3),
    ]


def with_factor3(m, slot):
    """an odd multiple of 3 next to m, below 2^slot"""
    m3 = m - m % 6 + 3
    if m3 >= 1 << slot:
        m3 -= 6
    assert m3 % 3 == 0 and m3 & 1 and 3 < m3 < 1 << slot
    return m3


def edge_cases(K32):
    """About 80 (name, y, m), 62 of them full-size, with 0 <= y < m, m odd and below 2^(32 K32): y = m - 2^k
    (which the binary GCD's sign fix answers) and its neighbours, over moduli with
    long runs of ones and zeros, short moduli and a square."""
    rnd = random.Random(9000 + K32)
    slot = 32 * K32
    cases = []

    def add(name, y, m):
        assert 0 <= y < m < 1 << slot and m & 1, name
        cases.append((name, y, m))

    for mname, m in edge_moduli(K32):
        bits = m.bit_length()
        if bits > 200:
            full = mname in ("odd", "nsq")
            ks = [1, 29, 30, 31, 59, 60, 61, bits // 2, bits - 2] if full else [30, 61, bits // 2]
            for k in ks:
                add("%s:m-2^%d" % (mname, k), m - (1 << k), m)
            add(mname + ":m-2", m - 2, m)
            add(mname + ":2^(bits/2)", 1 << (bits // 2), m)
            k = rnd.choice([k for k in range(2, bits) if m >> k & 1])   # a set bit: y stays below m
            add("%s:m^2^%d" % (mname, k), m ^ (1 << k), m)
            if full:
                add(mname + ":(m+1)/2", (m + 1) // 2, m)
                add(mname + ":2^210", 1 << 210, m)
                add(mname + ":0", 0, m)
                add(mname + ":1", 1, m)
            # a non-unit (about one in three of them also ends a step at or above m: mdiv's subtraction)
            m3 = m if m % 3 == 0 else with_factor3(m, slot)
            add(mname + ":shares3", 3 * rnd.randrange(1, m3 // 3), m3)
        elif bits > 2:                     # the 61-bit modulus: the nbits = 62 clamp from the first step
            for k in (1, 29, 30, 31, 58, 59):
                add("%s:m-2^%d" % (mname, k), m - (1 << k), m)
            add(mname + ":(m+1)/2", (m + 1) // 2, m)
            add(mname + ":0", 0, m)
            add(mname + ":1", 1, m)
            m3 = with_factor3(m, slot)
            add(mname + ":shares3", 3 * rnd.randrange(1, m3 // 3), m3)
            for t in range(4):             # plain values: five outer steps each
                add("%s:random%d" % (mname, t), rnd.randrange(m), m)
        else:                              # m = 3
            for y in (0, 1, 2):
                add("%s:%d" % (mname, y), y, m)
    return cases
