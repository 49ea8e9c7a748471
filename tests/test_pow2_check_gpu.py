"""pow2_check_kernel (csrc/pow2.hip), the 2-adic half of every even-modulus ring-Pedersen
and composite-DLog verdict, row by row through its parity entry Context.pow2_check
(fsdkr_pow2_check) against Python integers:

    (pow(a, ea, 2**k) * pow(b, eb, 2**k) - c * (d if used else 1)) % 2**k == 0

Every row's byte is compared by exact equality.  The rows are the smallest inputs that
reach each path of the kernel; each carries a label of the path it was built for, and
the conditions on the inputs (both verdicts per launch and per path) are asserted on the
CPU before the device call.

Widths: k = 1 .. 5, 31 .. 33, 63 .. 65, 2047, 2048, 3071, 3072 and four random ones,
mixed in one launch (a wave holds rows of many widths).
Odd bases 1, 2^k - 1, 3, 5, random with exponents 0, 1, 2^(k-3), 2^(k-2), 2^(k-2) + 1,
one of k + 30 bits and one of 20 bits: 3 and 5 have full order 2^(k-2), so e = 2^(k-3)
must give 1 + 2^(k-1) and e = 2^(k-2) must give 1 (the order cut min(eb, k - 2)).
Even bases with 1, 2 and k - 1 trailing zeros, base 0 and a nonzero multiple of 2^k,
with e tz on both sides of k, e = 8191, 8192, 2^32 + 1 (low limb 1) and 0.
Right-hand sides: the true c; c with one bit flipped in every limb of K and at bit
k - 1 (verdict 0); c with a bit flipped at k and above (outside the modulus: verdict
1); d through a set sel bit, a clear one, no sel, d absent, and the two wrong pairings
(c for d used where the bit is clear, c for d unused where it is set); sel bits in
words 0, 1 and 5 of sel_bits.
Row geometry: 97-limb rows (longer than K at every width: cut at 2^k), 1- to 3-limb rows
(zero-extended), the ring-Pedersen shape (a, ea, c, d with sel; no b, eb) and the DLog
shape (a, ea, b, eb of 8 limbs, c; no d), launches of 1, 64, 65 and 129 rows whose
verdicts are not periodic in 64.

Long exponents (more than a few hundred bits) stay on the rows that need them, and
the Python powers are memoised: the rows of one left-hand side share them."""
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 2047, 2048, 3071, 3072]
LONG = 97                      # limbs of the long rows: above K = 96 of k = 3072
SEL_WORDS = 6

_pow = functools.lru_cache(maxsize=None)(pow)


def expected(r, sel_bits):
    """The reference, written out: one row's verdict from Python integers."""
    k = r["k"]
    a, b, c = (1 if r[x] is None else r[x] for x in ("a", "b", "c"))
    ea, eb = (0 if r[x] is None else r[x] for x in ("ea", "eb"))
    d = r["d"]
    used = d is not None and (r["sel"] is None or (sel_bits[r["sel"] >> 5] >> (r["sel"] & 31)) & 1 == 1)
    return int((_pow(a, ea, 2 ** k) * _pow(b, eb, 2 ** k) - c * (d if used else 1)) % 2 ** k == 0)


def widths():
    rnd = random.Random("pow2-widths")
    return WIDTHS + [rnd.randrange(6, 31), rnd.randrange(66, 200), rnd.randrange(200, 2047), rnd.randrange(2049, 3071)]


def sel_words():
    rnd = random.Random("pow2-sel")
    return [rnd.getrandbits(32) | 1 << 7 for _ in range(SEL_WORDS)]     # every word has both values


def sel_index(sel_bits, word, value, rnd):
    while True:
        s = 32 * word + rnd.randrange(32)
        if (sel_bits[s >> 5] >> (s & 31)) & 1 == value:
            return s


def powers(k, rnd):
    """[(path, base, exponent)] for one width: every branch of pow_mod2k."""
    m = 1 << k
    out = []
    odd = [("odd-1", 1), ("odd-minus1", m - 1), ("odd-3", 3 % m), ("odd-5", 5 % m), ("odd-random", rnd.getrandbits(k) | 1)]
    exps = [("e0", 0), ("e1", 1), ("e-long", rnd.getrandbits(k + 30) | 1 << (k + 29)), ("e-short", rnd.getrandbits(20) | 1 << 19)]
    if k >= 3:
        exps.append(("e-half-order", 1 << (k - 3)))
    if k >= 2:
        exps += [("e-order", 1 << (k - 2)), ("e-order+1", (1 << (k - 2)) + 1)]
    for bn, b in odd:
        for en, e in exps:
            out.append((f"{bn}/{en}", b, e))
    if k >= 4:          # the sharp inputs of the order cut: 3 and 5 have order exactly 2^(k-2)
        for g in (3, 5):
            assert pow(g, 1 << (k - 3), m) == 1 + (1 << (k - 1)) and pow(g, 1 << (k - 2), m) == 1
    for tz in sorted({1, 2, k - 1} - {0}):
        if tz >= k:
            continue    # k = 1, 2: such a base is 0 mod 2^k, the zero-base rows below
        b = ((rnd.getrandbits(k) | 1) << tz) % m
        assert b and (b & -b) == 1 << tz
        es = {(k - 1) // tz, -(-(k - 1) // tz), k // tz, -(-k // tz), (k + 1) // tz, -(-(k + 1) // tz)} - {0}
        for e in sorted(es):
            side = "below" if e * tz < k else "at-or-above"
            out.append((f"even-tz{'K' if tz == k - 1 and tz > 2 else tz}/{side}", b, e))
        for en, e in (("e0", 0), ("e8191", 8191), ("e8192", 8192), ("e-2^32+1", (1 << 32) + 1)):
            out.append((f"even-tz{'K' if tz == k - 1 and tz > 2 else tz}/{en}", b, e))
    for en, e in (("e0", 0), ("e1", 1), ("e-2^32+1", (1 << 32) + 1)):
        out.append((f"zero/{en}", 0, e))
        out.append((f"multiple-of-2^k/{en}", (2 * rnd.randrange(1, 1 << 15) + 1) << k, e))
    return out


D_KINDS = ["d-sel-set", "d-sel-clear", "d-always", "d-absent"]


def rhs(kind, v, k, sel_bits, rnd, word):
    """(c, d, sel) with c d' == v (mod 2^k) for the d handling `kind`."""
    m = 1 << k
    if kind == "d-absent":
        return v, None, None
    d = rnd.getrandbits(k) | 1
    if kind == "d-sel-clear":       # d is not used: an even one, so a kernel that used it is wrong for odd v
        return v, (d + 1) % m if k > 1 else 0, sel_index(sel_bits, word, 0, rnd)
    c = v * pow(d, -1, m) % m
    return c, d, (None if kind == "d-always" else sel_index(sel_bits, word, 1, rnd))


def long_rows():
    """Every path at every width, in rows of LONG limbs (all operands cut at 2^k)."""
    rnd = random.Random("pow2-long")
    sel_bits = sel_words()
    rows = []
    n = 0
    for k in widths():
        m = 1 << k
        K = (k + 31) // 32
        specs = powers(k, rnd)
        for path, base, e in specs:
            n += 1
            # the other factor: absent, or an odd base to a short exponent; the two sides swap roles
            ob, oe = (None, None) if n % 3 == 0 else (rnd.getrandbits(k) | 1, rnd.getrandbits(9))
            side = "a" if n % 2 else "b"
            lhs = dict(a=base, ea=e, b=ob, eb=oe) if side == "a" else dict(a=ob, ea=oe, b=base, eb=e)
            v = _pow(base, e, m) * _pow(1 if ob is None else ob, oe or 0, m) % m
            kind = D_KINDS[n % 4]
            word = (0, 1, 5)[n % 3]
            c, d, sel = rhs(kind, v, k, sel_bits, rnd, word)
            # bits of c above k are outside the modulus: junk there on every other true row
            junk = (rnd.getrandbits(32 * LONG - k) << k) if n % 2 else 0
            rows.append(dict(lhs, c=c | junk, d=d, sel=sel, k=k, path=f"{side}:{path}", rhs=kind))
            # one wrong row per left-hand side
            wrong = n % 4
            d2 = rnd.getrandbits(k) | 1
            if wrong == 3 and (v % 2 == 0 or d2 % m == 1):
                wrong = 2       # c d2 == c would hold: v even (possibly 0) or d2 == 1
            if wrong == 0:
                bad = dict(c=c ^ 1, d=d, sel=sel, rhs="flip-bit0")
            elif wrong == 1:
                bad = dict(c=c ^ 1 << (k - 1), d=d, sel=sel, rhs="flip-top")
            elif wrong == 2:
                bad = dict(c=c ^ 1 << rnd.randrange(k), d=d, sel=sel, rhs="flip-random")
            else:           # the d pairing the other way round: c d where d is unused, c alone where it is used
                if n % 8 == 3:
                    bad = dict(c=v * pow(d2, -1, m) % m, d=d2, sel=sel_index(sel_bits, word, 0, rnd), rhs="wrong-d-unused")
                else:
                    bad = dict(c=v, d=d2, sel=sel_index(sel_bits, word, 1, rnd), rhs="wrong-d-used")
            rows.append(dict(lhs, k=k, path=f"{side}:{path}", **bad))
        # one cheap full-width left-hand side: a flip in every limb of K and at bit k - 1 (0), at k and above (1)
        g, e = 3 % m, rnd.getrandbits(20) | 1 << 19
        v = pow(g, e, m)
        for j in range(K):
            bit = min(32 * j + rnd.randrange(32), k - 1) if j == K - 1 else 32 * j + rnd.randrange(32)
            rows.append(dict(a=g, ea=e, b=None, eb=None, c=v ^ 1 << bit, d=None, sel=None, k=k, path="flips", rhs="flip-limb"))
        rows.append(dict(a=g, ea=e, b=None, eb=None, c=v ^ 1 << (k - 1), d=None, sel=None, k=k, path="flips", rhs="flip-top"))
        for bit in sorted({k, k + 1, 32 * K - 1, 32 * K, 32 * LONG - 1} - set(range(k))):
            rows.append(dict(a=g, ea=e, b=None, eb=None, c=v ^ 1 << bit, d=None, sel=None, k=k, path="flips", rhs="flip-above-k"))
        for _ in range(K // 2):       # true rows beside the flipped ones: random bits above k, all of them, none
            hi = rnd.choice([rnd.getrandbits(32 * LONG - k), (1 << (32 * LONG - k)) - 1, 0])
            rows.append(dict(a=g, ea=e, b=None, eb=None, c=v | hi << k, d=None, sel=None, k=k, path="flips", rhs="true-junk-above-k"))
    random.Random("pow2-long-order").shuffle(rows)
    return rows, sel_bits, (LONG,) * 6


def short_rows():
    """Operand rows of 1 to 3 limbs at every width: zero-extended where K is larger, cut where it is smaller."""
    rnd = random.Random("pow2-short")
    sel_bits = sel_words()
    rows = []
    n = 0
    for k in widths():
        for _ in range(6):
            n += 1
            a, b, ea, eb = rnd.getrandbits(16) | 1 << 15, rnd.getrandbits(16) | 1 << 15, rnd.randrange(1, 4), rnd.randrange(0, 3)
            if n % 3 == 0:
                a &= ~1
            true = a ** ea * b ** eb                    # below 2^80: the exact integer fits c's 3 limbs
            kind = ("d-absent", "d-sel-clear")[n % 2]
            d, sel = (None, None) if kind == "d-absent" else (rnd.getrandbits(32) | 1, sel_index(sel_bits, n % 3, 0, rnd))
            rows.append(dict(a=a, ea=ea, b=b, eb=eb, c=true, d=d, sel=sel, k=k, path="short", rhs=kind))
            rows.append(dict(a=a, ea=ea, b=b, eb=eb, c=true ^ 1 << rnd.randrange(min(k, 80)), d=d, sel=sel, k=k,
                             path="short", rhs="flip-random"))
            # d used: a = c d as integers, so the check holds at every width
            c, d = rnd.getrandbits(16) | 1, rnd.getrandbits(16) | 1
            sel = (None, sel_index(sel_bits, n % 3, 1, rnd))[n % 2]
            rows.append(dict(a=c * d, ea=1, b=None, eb=None, c=c, d=d, sel=sel, k=k, path="short", rhs="d-used"))
            rows.append(dict(a=c * d, ea=1, b=None, eb=None, c=c ^ 1, d=d, sel=sel, k=k, path="short", rhs="flip-bit0"))
    return rows, sel_bits, (1, 1, 1, 1, 3, 1)


def ring_pedersen_rows():
    """T^Z == A S^e: a, ea, c, d with sel as fsdkr_ring_pedersen_verify and collect() build them
    (64-limb T, A, S, Z of 65 limbs), no b / eb; widths up to 2047 as N = 2^k m < 2^2048."""
    rnd = random.Random("pow2-rp")
    sel_bits = sel_words()
    rows = []
    n = 0
    for k in [w for w in widths() if w <= 2047]:
        m = 1 << k
        for T in (rnd.getrandbits(2048) | 1, rnd.getrandbits(2047) << 1 | 2, rnd.getrandbits(2048 - k) << k):
            S = rnd.getrandbits(2048) | 1
            for zbits in (2080, 200, 9):
                n += 1
                Z = rnd.getrandbits(zbits) | 1 << (zbits - 1)
                bit = n % 2
                v = pow(T, Z, m)
                A = (v * pow(S, -bit, m) % m) | (rnd.getrandbits(2048 - k) << k)
                sel = sel_index(sel_bits, (0, 1, 5)[n % 3], bit, rnd)
                rows.append(dict(a=T, ea=Z, b=None, eb=None, c=A, d=S, sel=sel, k=k, path="rp", rhs=f"bit{bit}"))
                flip = n % 4 < 2 or v * (S - 1) % m == 0        # the other bit's d gives the same product
                bad = (A ^ 1 << rnd.randrange(k), sel) if flip else (A, sel_index(sel_bits, n % 3, 1 - bit, rnd))
                rows.append(dict(a=T, ea=Z, b=None, eb=None, c=bad[0], d=S, sel=bad[1], k=k, path="rp",
                                 rhs="flip-random" if flip else "wrong-bit"))
    return rows, sel_bits, (64, 65, 1, 1, 64, 64)


def dlog_rows():
    """g^y ni^e == x: a, ea, b, eb of 8 limbs, c, no d, as collect() builds them (y of 72 limbs)."""
    rnd = random.Random("pow2-dlog")
    rows = []
    n = 0
    for k in [w for w in widths() if w <= 2047]:
        m = 1 << k
        for ybits in (2300, 180):
            n += 1
            g, ni = rnd.getrandbits(2048) | 1, rnd.getrandbits(2048) | 1     # gcd(g, N) = 1: odd
            y, e = rnd.getrandbits(ybits) | 1 << (ybits - 1), rnd.getrandbits(256) | 1 << 255
            x = pow(g, y, m) * pow(ni, e, m) % m | (rnd.getrandbits(2048 - k) << k)
            rows.append(dict(a=g, ea=y, b=ni, eb=e, c=x, d=None, sel=None, k=k, path="dlog", rhs="true"))
            bad = x ^ 1 << (k - 1) if n % 2 else x ^ 1 << rnd.randrange(k)
            wrong_e = n % 4 == 0 and k >= 300       # ni^(2^255) != 1 needs k - 2 well above 255
            rows.append(dict(a=g, ea=y, b=ni, eb=e ^ wrong_e << 255, c=x if wrong_e else bad, d=None, sel=None, k=k,
                             path="dlog", rhs="wrong-e-top-limb" if wrong_e else "flip"))
    return rows, [], (64, 72, 64, 8, 64, 1)


def conditions(rows, want, single_verdict=()):
    """Conditions on the inputs, checked before the device call: a quarter of each verdict
    in the launch, and both verdicts on every path and every right-hand-side kind that can
    have both."""
    assert len(rows) == len(want)
    ones = sum(want)
    assert 4 * ones >= len(want) and 4 * (len(want) - ones) >= len(want), (ones, len(want))
    by_path, by_rhs = {}, {}
    for r, w in zip(rows, want):
        by_path.setdefault(r["path"], set()).add(w)
        by_rhs.setdefault(r["rhs"], set()).add(w)
    one_sided = [p for p, s in by_path.items() if s != {0, 1}]
    assert not one_sided, one_sided
    for kind, s in by_rhs.items():
        if kind.startswith(("flip-above", "true")) or kind in ("d-used",):
            assert s == {1}, (kind, s)
        elif kind.startswith(("flip", "wrong")):
            # a flipped bit below k always changes the residue; the wrong pairings are only
            # built where they change it
            assert s == {0}, (kind, s)
        else:
            assert 1 in s, (kind, s)
    for kind in single_verdict:
        assert kind in by_rhs, kind


def run(ctx, rows, sel_bits, lens):
    got = ctx.pow2_check(*([r[x] for r in rows] for x in ("a", "ea", "b", "eb", "c", "d")), [r["k"] for r in rows],
                         lens, sel=[r["sel"] for r in rows], sel_bits=sel_bits).tolist()
    return got


def compare(rows, want, got, what):
    bad = [i for i, (w, g) in enumerate(zip(want, got)) if w != g]
    print(f"{what}: {len(rows)} rows, {sum(want)} expected 1, {len(bad)} differ")
    if bad:
        r = rows[bad[0]]
        paths = sorted({(rows[i]["path"], rows[i]["rhs"], rows[i]["k"]) for i in bad})
        detail = ", ".join(f"{x}={'None' if r[x] is None else hex(r[x])}" for x in ("a", "ea", "b", "eb", "c", "d"))
        raise AssertionError(f"{what}: {len(bad)} of {len(rows)} rows differ; first row {bad[0]}: k={r['k']} "
                             f"path={r['path']} rhs={r['rhs']} sel={r['sel']} expected {want[bad[0]]} got {got[bad[0]]}; "
                             f"{detail}; all (path, rhs, k): {paths[:40]}")


@pytest.fixture(scope="module")
def sets():
    """The row sets and their expected verdicts, built once and left unchanged."""
    out = {}
    for name, make in (("long", long_rows), ("short", short_rows), ("rp", ring_pedersen_rows), ("dlog", dlog_rows)):
        rows, sel_bits, lens = make()
        out[name] = (rows, sel_bits, lens, [expected(r, sel_bits) for r in rows])
    return out


@pytest.mark.parametrize("name", ["long", "short", "rp", "dlog"])
def test_rows_against_python_integers(gpu_ctx, sets, name):
    rows, sel_bits, lens, want = sets[name]
    conditions(rows, want)
    ks = {r["k"] for r in rows}
    assert ks >= {w for w in WIDTHS if name in ("long", "short") or w <= 2047}
    if name == "long":
        kinds = {r["rhs"] for r in rows}
        assert kinds >= set(D_KINDS) | {"flip-bit0", "flip-top", "flip-random", "flip-limb", "flip-above-k",
                                        "wrong-d-unused", "wrong-d-used"}
        assert {(r["sel"] >> 5) for r in rows if r["sel"] is not None} >= {0, 1, 5}
        # every path of powers() at the largest width, on either side
        assert {r["path"].split(":")[-1] for r in rows if r["k"] == 3072} >= {p for p, _, _ in powers(3072, random.Random(0))}
    got = run(gpu_ctx, rows, sel_bits, lens)
    compare(rows, want, got, name)


@pytest.mark.parametrize("count", [1, 64, 65, 129])
def test_launch_sizes(gpu_ctx, sets, count):
    """Rows of small widths drawn so that the verdicts are not periodic in 64: a row mapped
    to the wrong thread or block shows.  A launch of one row cannot hold both verdicts:
    it runs twice, once with each."""
    rows, sel_bits, lens, want = sets["long"]
    rnd = random.Random(f"pow2-count-{count}")
    pool = [i for i, r in enumerate(rows) if r["k"] <= 65]
    if count == 1:
        picks = [[next(i for i in pool if want[i] == v)] for v in (1, 0)]
    else:
        while True:
            idx = rnd.sample(pool, count)
            w = [want[i] for i in idx]
            if 4 * sum(w) >= count and 4 * (count - sum(w)) >= count and (count <= 64 or any(w[i] != w[i + 64] for i in range(count - 64))):
                break
        picks = [idx]
        assert w != [w[0]] * count
    for idx in picks:
        sub = [rows[i] for i in idx]
        got = run(gpu_ctx, sub, sel_bits, lens)
        compare(sub, [want[i] for i in idx], got, f"count {count}")


def test_absent_operands(gpu_ctx):
    """Address 0 stands for the value 1 (exponent 0): each operand absent in turn, over a row
    whose limbs would change the verdict if they were read."""
    k = 40
    m = 1 << k
    full = dict(a=3, ea=5, b=7, eb=2, c=243 * 49 * pow(11, -1, m) % m, d=11, sel=None, k=k)
    rows = [full]
    for x in ("a", "ea", "b", "eb", "c", "d"):
        rows.append(dict(full, **{x: None}))
    rows += [dict(a=None, ea=None, b=None, eb=None, c=None, d=None, sel=None, k=k),            # 1 == 1
             dict(a=None, ea=9, b=None, eb=9, c=None, d=None, sel=None, k=k),                  # 1^9 1^9 == 1
             dict(a=3, ea=None, b=7, eb=None, c=1, d=None, sel=None, k=k),                     # x^0 == 1
             dict(a=0, ea=None, b=0, eb=0, c=1, d=None, sel=None, k=k),                        # 0^0 == 1
             dict(a=3, ea=5, b=None, eb=None, c=243, d=0, sel=0, k=k),                         # d = 0 behind a clear bit
             dict(a=3, ea=5, b=None, eb=None, c=243, d=0, sel=1, k=k)]                         # and behind a set one
    sel_bits = [2]
    for r in rows:
        r.setdefault("path", "absent")
        r.setdefault("rhs", "absent")
    want = [expected(r, sel_bits) for r in rows]
    assert want == [1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0]
    got = run(gpu_ctx, rows, sel_bits, (1, 1, 1, 1, 2, 1))
    compare(rows, want, got, "absent operands")


def test_refusals(gpu_ctx):
    from fsdkr import _native
    from fsdkr._native import FsdkrError

    def refused(k, sel=None, sel_bits=None, lens=(1,) * 6):
        with pytest.raises(FsdkrError) as e:
            gpu_ctx.pow2_check([3], [1], [1], [1], [3], [1], [k], lens, sel=sel, sel_bits=sel_bits)
        return e.value.code
    assert refused(0) == _native.FSDKR_E_ARG
    assert refused(3073) == _native.FSDKR_E_ARG
    assert refused(8, sel=[32], sel_bits=[1]) == _native.FSDKR_E_ARG        # past the one word
    assert refused(8, sel=[0], sel_bits=None) == _native.FSDKR_E_ARG        # no sel_bits at all
    one = np.ones(1, dtype=np.uint32)
    out = np.zeros(1, dtype=np.uint8)
    p, o = _native._ptr(one), out.ctypes.data_as(_native.u8p)
    lib = gpu_ctx._lib
    assert lib.fsdkr_pow2_check(gpu_ctx.handle, 1, p, 1, p, 1, p, 0, p, 1, p, 1, p, 1, p, None, None, None, 0, o) == _native.FSDKR_E_ARG
    assert lib.fsdkr_pow2_check(gpu_ctx.handle, 1, p, 1, p, 1, None, 1, p, 1, p, 1, p, 1, p, None, None, None, 0, o) == _native.FSDKR_E_ARG
    assert lib.fsdkr_pow2_check(gpu_ctx.handle, 1, p, 1, p, 1, p, 1, p, 1, p, 1, p, 1, p, None, None, None, 0, o) == _native.FSDKR_OK
    assert out.tolist() == [1]
    assert gpu_ctx.pow2_check([3], [1], [1], [1], [3], [1], [8], (1,) * 6, sel=[31], sel_bits=[1 << 31]).tolist() == [1]
    assert gpu_ctx.pow2_check([3], [1], [1], [1], [3], [1], [3072], (1,) * 6).tolist() == [1]
    assert gpu_ctx.pow2_check([], [], [], [], [], [], [], (1,) * 6).tolist() == []
    with pytest.raises(ValueError):
        gpu_ctx.pow2_check([1 << 32], [1], [1], [1], [3], [1], [8], (1,) * 6)
