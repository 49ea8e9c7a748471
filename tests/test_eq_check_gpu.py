"""eq_check_kernel (csrc/vmont.hip) through its parity entry Context.eq_check
(fsdkr_eq_check): the kernel that turns a*b == c*d (mod N) [and c < N] into the one
bit every ring-Pedersen, PDL u2 / u3, correct-key and DLog verdict is made of.

The expected verdict is always Python's (a*b - c*d) % N == 0 and (not flag or c < N).
Whole proofs cannot tell a kernel that compares every digit from one that compares
some: a tampered proof value changes every digit of the compared residues.  Here
the two sides are chosen digit by digit.  With b = d = R mod N (R = 2^(29 KD)) the
kernel's two Montgomery products are exactly a and c, so a and c that differ in one
radix-2^29 digit of one lane must be told apart by that lane alone.

SHAPES mirrors the launch table of vmont.hip: KD digits over G lanes, L = KD / G
digits per lane, BLOCK / G = 256 / G instances per block."""
import ctypes
import functools

import pytest

from oracle.rng import Rng

pytestmark = pytest.mark.gpu

SHAPES = {64: (72, 8), 96: (108, 4), 128: (144, 8), 192: (216, 8)}   # K32 -> (KD, G)
WIDTHS = sorted(SHAPES)
COUNTS = [1, 31, 33, 65, 257]   # around the 32 (8 lanes) and 64 (4 lanes) instances of a block
LANES = [(K, j) for K in WIDTHS for j in range(SHAPES[K][1])]


def geom(K):
    KD, G = SHAPES[K]
    return KD, G, KD // G, 1 << (29 * KD)


def digits(v, KD):
    return [(v >> (29 * k)) & ((1 << 29) - 1) for k in range(KD)]


def verdict(a, b, c, d, N, flag=0):
    return int((a * b - c * d) % N == 0 and (not flag or c < N))


@functools.lru_cache(maxsize=None)
def full_modulus(K, tag="n"):
    """A full-width odd N with its top bit set."""
    return Rng(("eq-check-mod", K, tag)).bits(32 * K) | (1 << (32 * K - 1)) | 1


def coprime(a, b):
    while b:
        a, b = b, a % b
    return a == 1


def unit(rng, N, low=1):
    """A unit modulo N in [low, N)."""
    while True:
        v = low + rng.sample_below(N - low)
        if coprime(v, N):
            return v


def run(ctx, K, rows, mods, sel_bits=None, lens=None):
    """rows: (a, b, c, d, modulus index, sel or None, flag).  Asserts the device's
    verdict of every row against Python's and returns the expected list."""
    want = []
    for a, b, c, d, mi, sel, flag in rows:
        if sel is not None and not (sel_bits[sel >> 5] >> (sel & 31)) & 1:
            d = 1
        want.append(verdict(a, b, c, d, mods[mi], flag))
    use_sel = any(r[5] is not None for r in rows)
    got = ctx.eq_check([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows],
                       mods, [r[4] for r in rows], K, lens=lens, sel=[r[5] for r in rows] if use_sel else None,
                       sel_bits=sel_bits, flags=[r[6] for r in rows]).tolist()
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    print(f"K32={K}: {len(rows)} rows, {sum(want)} expected 1, wrong (row, got, want): {wrong[:16]}")
    assert not wrong, f"{len(wrong)} of {len(rows)} verdicts differ; first (row, got, want): {wrong[:16]}"
    return want


def one_digit_pair(rng, N, KD, pos):
    """x in [N/2, N) with bit pos set and y = x - 2^pos: equal in every digit but one."""
    delta = 1 << pos
    assert 2 * delta < N
    while True:
        x = (N // 2 + rng.sample_below(N - N // 2)) | delta
        if x < N:
            break
    y = x - delta
    dx, dy = digits(x, KD), digits(y, KD)
    assert [k for k in range(KD) if dx[k] != dy[k]] == [pos // 29] and N // 2 - delta <= y < x < N
    return x, y


def lane_positions(K, j):
    """Bit positions tested in lane j: bits 0 and 28 of its first, middle and last digit,
    those with 2^pos < N/2 for a full-width N; in the top lane also the highest such bit."""
    KD, G, L, _ = geom(K)
    pos = [29 * (j * L + i) + bit for i in (0, L // 2, L - 1) for bit in (0, 28)]
    if j == G - 1:
        pos.append(32 * K - 3)
    pos = [p for p in pos if p <= 32 * K - 3]
    assert len(pos) >= 3 and all(p // 29 // L == j for p in pos)
    return pos


# ---- one differing digit, every lane -----------------------------------------------
@pytest.mark.parametrize("K,lane", LANES, ids=[f"{K}-lane{j}" for K, j in LANES])
def test_one_differing_digit(gpu_ctx, K, lane):
    KD, G, L, R = geom(K)
    N = full_modulus(K)
    rng = Rng(("eq-one-digit", K, lane))
    rn = R % N
    rows = []
    for pos in lane_positions(K, lane):
        x, y = one_digit_pair(rng, N, KD, pos)
        rows += [(x, rn, y, rn, 0, None, 0), (x, rn, x, rn, 0, None, 0)]
    assert run(gpu_ctx, K, rows, [N]) == [0, 1] * (len(rows) // 2)


# ---- the two sides agree below a lane boundary and differ above it ------------------
@pytest.mark.parametrize("K", WIDTHS)
def test_difference_above_a_lane_boundary(gpu_ctx, K):
    KD, G, L, R = geom(K)
    N = full_modulus(K)
    rng = Rng(("eq-boundary", K))
    rn = R % N
    rows = []
    for k in [2] + [k for k in range(1, G) if k != 2]:
        x = N // 2 + rng.sample_below(N - N // 2)
        y = x % (1 << (29 * k * L))
        assert y != x and digits(x, KD)[:k * L] == digits(y, KD)[:k * L]
        rows += [(x, rn, y, rn, 0, None, 0), (x, rn, x, rn, 0, None, 0)]
    assert run(gpu_ctx, K, rows, [N]) == [0, 1] * (G - 1)


# ---- random relations ---------------------------------------------------------------
def relation_moduli(K):
    rng = Rng(("eq-rel-mod", K))
    return [full_modulus(K), (1 << (32 * K)) - 1, rng.bits(32 * K - 61) | (1 << (32 * K - 62)) | 1,
            full_modulus(K, "second"), rng.bits(32 * K - 1) | (1 << (32 * K - 2)) | 1]


@pytest.mark.parametrize("K", WIDTHS)
def test_random_relations(gpu_ctx, K):
    """200 true relations a b = c d over 5 moduli (2^bits - 1 and one 61 bits short among
    them; a anywhere in the slot), and for each c + 1, c with one bit flipped (the bit
    moving over the whole width) and N - c."""
    mods = relation_moduli(K)
    assert mods[1].bit_length() == 32 * K and mods[2].bit_length() == 32 * K - 61
    rng = Rng(("eq-relations", K))
    rows = []
    for i in range(200):
        mi = i % 5
        N = mods[mi]
        a, b = rng.bits(32 * K), rng.sample_below(N)
        d = unit(rng, N)
        c = a * b * pow(d, -1, N) % N
        p = (i * 32 * K) // 200 + (i % 7)
        rows += [(a, b, c, d, mi, None, 0), (a, b, c + 1, d, mi, None, 0), (a, b, c ^ (1 << p), d, mi, None, 0),
                 (a, b, N - c, d, mi, None, 0)]
    want = run(gpu_ctx, K, rows, mods)
    assert want[0::4] == [1] * 200 and sum(want) <= 210


# ---- unreduced operands on the edge of the precondition -------------------------------
def edge_moduli(K):
    rng = Rng(("eq-edge-mod", K))
    return [full_modulus(K), rng.bits(16 * K) | (1 << (16 * K - 1)) | 1, 3]


@pytest.mark.parametrize("K", WIDTHS)
def test_unreduced_operands(gpu_ctx, K):
    """a = 2^(32 K32) - 1 against b < N, and c = c0 + k N up to the end of the slot against
    d < N (likewise d = d0 + k N against c0): each product stays below R N, where one
    conditional subtraction still reduces it.  Over a full-width N, a half-width N in
    the wide slot, and N = 3."""
    top = (1 << (32 * K)) - 1
    mods = edge_moduli(K)
    rng = Rng(("eq-unreduced", K))
    rows = []
    for mi, N in enumerate(mods):
        for b in [1, N - 1, rng.sample_below(N), rng.sample_below(N)]:
            d = unit(rng, N)
            c0 = top * b * pow(d, -1, N) % N
            kmax = (top - c0) // N
            ks = sorted({min(1, kmax), kmax // 2, kmax})
            for k in ks:
                rows.append((top, b, c0 + k * N, d, mi, None, 0))
                rows.append((b, top, c0 + k * N, d, mi, None, 0))
            rows.append((top, b, c0, d + ((top - d) // N) * N, mi, None, 0))
            if c0 + kmax * N < top:
                rows.append((top, b, c0 + kmax * N + 1, d, mi, None, 0))
    want = run(gpu_ctx, K, rows, mods)
    assert sum(want) >= len(rows) - 12 and 0 in want


# ---- the c < N flag -----------------------------------------------------------------
def flag_rows(K, N, mi, rng):
    def a_for(c, b, d):
        return c * d * pow(b, -1, N) % N
    top = 1 << (32 * K)
    rows = []
    b, d = unit(rng, N), unit(rng, N)
    c0 = rng.sample_below(min(N, top - N))
    a = a_for(c0, b, d)
    rows += [(a, b, c0, d, mi, None, 1), (a, b, c0 + N, d, mi, None, 1), (a, b, c0 + N, d, mi, None, 0),
             (0, b, N, d, mi, None, 1), (0, b, N, d, mi, None, 0),
             (a_for(N - 1, b, d), b, N - 1, d, mi, None, 1), (a, b, N - 1, d, mi, None, 1)]
    # c on both sides of N, away from it only in the last digit that holds bits of N
    step = 1 << (29 * ((N.bit_length() - 1) // 29))
    assert step < N and N + step < top
    for c in (N - step, N + step):
        dc, dn = digits(c, SHAPES[K][0]), digits(N, SHAPES[K][0])
        assert [k for k in range(len(dn)) if dc[k] != dn[k]] == [(N.bit_length() - 1) // 29]
        rows += [(a_for(c, b, d), b, c, d, mi, None, 1), (a_for(c, b, d), b, c, d, mi, None, 0)]
    return rows


@pytest.mark.parametrize("K", WIDTHS)
def test_c_below_n_flag(gpu_ctx, K):
    rng = Rng(("eq-flag", K))
    # a top digit of N that is neither all ones nor zero, so N +- one unit of it stays in the slot
    N = full_modulus(K) & ~(1 << (32 * K - 2))
    half = edge_moduli(K)[1]
    rows = flag_rows(K, N, 0, rng) + flag_rows(K, half, 1, rng)
    want = run(gpu_ctx, K, rows, [N, half])
    assert want[:7] == [1, 0, 1, 0, 1, 1, 0] and want[7:11] == [1, 1, 0, 1]


@pytest.mark.parametrize("K", WIDTHS)
def test_c_wider_than_the_modulus(gpu_ctx, K):
    """c rows of K32 + 2 limbs under the flag: zero limbs above K32 change nothing, a
    nonzero one gives 0 -- also where the relation holds (c = c0 + 2^40 N, below R, so
    both products agree) and where the kernel's digits cannot see it (a bit above R)."""
    KD, G, L, R = geom(K)
    N = full_modulus(K)
    rng = Rng(("eq-wide-c", K))
    b, d = N - 2, N - 1
    c0 = rng.sample_below(N)
    a = c0 * d * pow(b, -1, N) % N
    wide = [c0 + (N << 40), c0 + (1 << (32 * K)), c0 + (1 << (32 * K + 33))]
    if 32 * (K + 2) - 1 >= 29 * KD:
        wide.append(c0 + (1 << (32 * (K + 2) - 1)))
    assert wide[0] < R and all(w >> (32 * K) for w in wide)
    rows = [(a, b, c0, d, 0, None, 1), (a, b, c0, d, 0, None, 0)] + [(a, b, w, d, 0, None, 1) for w in wide]
    want = run(gpu_ctx, K, rows, [N], lens=(K, K, K + 2, K))
    assert want == [1, 1] + [0] * len(wide)


# ---- sel: d or the constant 1 by a bit of sel_bits -------------------------------------
@pytest.mark.parametrize("K", WIDTHS)
def test_sel_bits(gpu_ctx, K):
    """Bit indices 0, 31, 32 and 95 of a three-word sel_bits at both values, their
    neighbours holding the opposite value; a relation that holds only with d = 1 and
    one that holds only with the stored d, under each."""
    N = full_modulus(K)
    rng = Rng(("eq-sel", K))
    idx = (0, 31, 32, 95)
    words = [0, 0, 0]
    for s, bit in zip(idx, (1, 0, 1, 0)):
        for t, v in ((s, bit), (s ^ 1, 1 - bit)):
            words[t >> 5] |= v << (t & 31)
    for sel_bits in (words, [w ^ 0xFFFFFFFF for w in words]):
        rows = []
        for s in idx + (None,):
            a, b = rng.sample_below(N), rng.sample_below(N)
            d = unit(rng, N, low=2)
            rows += [(a, b, a * b % N, d, 0, s, 0), (a, b, a * b * pow(d, -1, N) % N, d, 0, s, 0)]
        want = run(gpu_ctx, K, rows, [N], sel_bits=sel_bits)
        for k, s in enumerate(idx):
            bit = (sel_bits[s >> 5] >> (s & 31)) & 1
            assert want[2 * k:2 * k + 2] == ([0, 1] if bit else [1, 0])
        assert want[8:] == [0, 1]


# ---- short rows -------------------------------------------------------------------------
@pytest.mark.parametrize("K", WIDTHS)
def test_short_rows(gpu_ctx, K):
    """Operand rows of 1, 8 and K32 - 1 limbs (every operand alike, then mixed lengths).
    Over a full-width N: a = p q, b = r s, c = p r, d = q s, each as wide as its row
    allows.  Over N = 2^31 - 1, where the short values wrap: a anywhere in its row,
    b, c, d reduced.  Negatives change one bit of c, anywhere in its row."""
    small = (1 << 31) - 1
    mods = [full_modulus(K), small]
    for lens in [(1,) * 4, (8,) * 4, (K - 1,) * 4, (1, K, 8, K - 1), (K - 1, 8, K, 1)]:
        la, lb, lc, ld = lens
        rng = Rng(("eq-short", K, lens))
        rows = []
        for i in range(34):
            if i % 2:
                a, b, d = rng.bits(32 * la), rng.sample_below(small), unit(rng, small)
                c = a * b * pow(d, -1, small) % small
            else:
                p, q = rng.bits(16 * min(la, lc)), rng.bits(16 * min(la, ld))
                r, s = rng.bits(16 * min(lb, lc)), rng.bits(16 * min(lb, ld))
                a, b, c, d = p * q, r * s, p * r, q * s
            rows += [(a, b, c, d, i % 2, None, 0), (a, b, c ^ (1 << ((61 * i) % (32 * lc))), d, i % 2, None, 0)]
        assert all(v.bit_length() <= 32 * n for r in rows for v, n in zip(r[:4], lens))
        want = run(gpu_ctx, K, rows, mods, lens=lens)
        assert want[0::2] == [1] * 34 and want[1::2] == [0] * 34


# ---- ragged launches ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_rows(K):
    """257 rows: positives, random negatives and one-digit negatives of every lane in
    turn; any prefix is closed by its own top-lane negative (ragged_launch)."""
    KD, G, L, R = geom(K)
    N = full_modulus(K)
    rng = Rng(("eq-ragged", K))
    rn = R % N
    rows = []
    for i in range(max(COUNTS)):
        pos = lane_positions(K, i % G)
        x, y = one_digit_pair(rng, N, KD, pos[i % len(pos)])
        rows.append([(x, rn, x, rn, 0, None, 0), (x, rn, y, rn, 0, None, 0), (x, rn, rng.sample_below(N), rn, 0, None, 0)][i % 3])
    return N, rows


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("K", WIDTHS)
def test_ragged_launch(gpu_ctx, K, count):
    KD, G, L, R = geom(K)
    N, rows = ragged_rows(K)
    x, y = one_digit_pair(Rng(("eq-ragged-last", K, count)), N, KD, 32 * K - 3)
    rows = rows[:count - 1] + [(x, R % N, y, R % N, 0, None, 0)]
    want = run(gpu_ctx, K, rows, [N])
    assert want[-1] == 0 and (count < 4 or (1 in want and want.count(0) >= count // 2))


# ---- refusals ------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    from fsdkr import _native
    from fsdkr._native import FsdkrError
    K, N = 64, full_modulus(64)
    top = (1 << 2048) - 1

    def refused(*args, **kw):
        with pytest.raises(FsdkrError) as e:
            gpu_ctx.eq_check(*args, **kw)
        return e.value.code
    assert refused([1], [1], [1], [1], [N + 1], [0], K) == _native.FSDKR_E_ARG          # even modulus
    assert refused([1], [1], [1], [1], [1], [0], K) == _native.FSDKR_E_ARG              # modulus 1
    assert refused([1], [1], [1], [1], [N], [1], K) == _native.FSDKR_E_ARG              # mod_idx out of range
    assert refused([N], [top], [1], [1], [N], [0], K) == _native.FSDKR_E_ARG            # a, b >= N
    assert refused([1], [1], [N], [N], [N], [0], K) == _native.FSDKR_E_ARG              # c, d >= N
    assert refused([1], [1], [5], [7], [3], [0], K) == _native.FSDKR_E_ARG              # the same, small N
    assert refused([1], [1], [1 << 2048], [1], [N], [0], K, lens=(K, K, K + 2, K)) == _native.FSDKR_E_ARG
    assert refused([1], [1], [1], [1], [N], [0], 80) == _native.FSDKR_E_UNSUPPORTED
    # d >= N is fine where the bit selects 1, and refused where it selects d
    assert gpu_ctx.eq_check([5], [1], [N + 5], [top], [N], [0], K, sel=[3], sel_bits=[0]).tolist() == [1]
    assert refused([5], [1], [N + 5], [top], [N], [0], K, sel=[3], sel_bits=[8]) == _native.FSDKR_E_ARG
    null = ctypes.cast(None, _native.u32p)
    assert gpu_ctx._lib.fsdkr_eq_check(gpu_ctx.handle, K, 0, null, K, null, K, null, K, null, K, null, null, null,
                                       null, 0, null, None) == _native.FSDKR_OK
    assert gpu_ctx.eq_check([], [], [], [], [N], [], K).tolist() == []
    # the context still works after the refusals
    assert gpu_ctx.eq_check([6, 6], [35, 35], [10, 11], [21, 21], [N], [0, 0], K).tolist() == [1, 0]
