"""CPU checks of Bob's prover on the constant-time entries:
fsdkr.mta.generate_bob(fused=True) and respond(fused_proofs=True) over a stand-in
context that serves the device calls with pow (draw order, instance order and
widths of the one pedersen_commit call, the one bob_commit_v call with gamma
reduced mod N and a_enc mod N^2, the ValueErrors, equality with the oracle's
prover), and a Python model of the 768-squaring tail's schedule
(csrc/mta_ct.hip bob_v_tail_ct_kernel) against pow."""
import math

import pytest

import mta_oracle as mo
from oracle import paillier
from oracle import secp256k1 as ec
from oracle.rng import Rng

Q = ec.Q
Q3 = Q ** 3


# ---- a stand-in context: the device calls by pow, recorded -------------------------
class PowContext:
    def __init__(self):
        self.calls = []

    def pedersen_commit(self, xs, ys, keys, key_idx, nl, xl=None, yl=None):
        self.calls.append(("pedersen_commit", dict(xs=list(xs), ys=list(ys), keys=list(keys), key_idx=list(key_idx),
                                                   nl=nl, xl=xl, yl=yl)))
        for x, y in zip(xs, ys):
            assert 0 <= x < 1 << (32 * xl) and 0 <= y < 1 << (32 * yl)
        return [pow(keys[i][1], x, keys[i][0]) * pow(keys[i][2], y, keys[i][0]) % keys[i][0]
                for x, y, i in zip(xs, ys, key_idx)]

    def bob_commit_v(self, a_encs, alphas, gammas, betas, ns, n_idx, nl, fused=True):
        self.calls.append(("bob_commit_v", dict(a_encs=list(a_encs), alphas=list(alphas), gammas=list(gammas),
                                                betas=list(betas), ns=list(ns), n_idx=list(n_idx), nl=nl, fused=fused)))
        out = []
        for a, al, ga, be, i in zip(a_encs, alphas, gammas, betas, n_idx):
            N = ns[i]
            assert 0 <= a < N * N and 0 <= al < 1 << 768 and 0 <= ga < N and 0 <= be < N
            out.append(pow(a, al, N * N) * (1 + ga * N) * pow(be, N, N * N) % (N * N))
        return out

    def mta_respond(self, a_encs, bs, beta_prims, rs, ns, n_idx, nl, fused=True):
        self.calls.append(("mta_respond", dict(count=len(a_encs), nl=nl)))
        return [pow(a, b, ns[i] ** 2) * (1 + bp * ns[i]) * pow(r, ns[i], ns[i] ** 2) % ns[i] ** 2
                for a, b, bp, r, i in zip(a_encs, bs, beta_prims, rs, n_idx)]

    def modexp_batch(self, bases, exps, mods, mod_idx, mod_limbs, secret=False):
        self.calls.append(("modexp_batch", dict(count=len(bases), nl=mod_limbs, secret=secret)))
        return [pow(b, e, mods[i]) for b, e, i in zip(bases, exps, mod_idx)]

    def ec_mul_g(self, scalars):
        self.calls.append(("ec_mul_g", dict(count=len(scalars))))
        return [ec.mul(ec.G, s) for s in scalars]


class LoggedRng:
    def __init__(self, seed):
        self.rng, self.bounds, self.values = Rng(seed), [], []

    def sample_below(self, upper):
        self.bounds.append(upper)
        self.values.append(self.rng.sample_below(upper))
        return self.values[-1]


@pytest.fixture(scope="module")
def small_keys():
    """Two 768-bit Paillier keys with a statement each (the 2048-bit class)."""
    rng = Rng("bob-prover-fused-cpu-keys")
    out = []
    for _ in range(2):
        ek, dk = paillier.keypair_with_modulus_size(768, rng)
        ekt, dkt = paillier.keypair_with_modulus_size(768, rng)
        out.append(dict(ek=ek, dk=dk, st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)))
    return out


def _items(small_keys, n, seed):
    items = []
    for k in range(n):
        key = small_keys[k % 2]
        a_enc, m, b, beta_prim, r = mo.mta_scenario(key["ek"], Rng((seed, k)))
        items.append((a_enc, m, b, beta_prim, key["ek"], key["st"], r))
    return items


def _calls(ctx, name):
    return [c[1] for c in ctx.calls if c[0] == name]


@pytest.mark.parametrize("check", [False, True])
def test_generate_bob_fused_over_pow(small_keys, check):
    from fsdkr import mta
    items = _items(small_keys, 5, "bob-prover-fused-cpu")
    b_edge, bp_edge = (1 << 256) - 1, items[3][4].n - 1      # the widest b and beta' that go through
    items[2] = items[2][:2] + (b_edge,) + items[2][3:]
    items[3] = items[3][:3] + (bp_edge,) + items[3][4:]
    for k in (2, 3):                                         # their mta_out follows
        a_enc, _, b, bp, ek, st, r = items[k]
        items[k] = (a_enc, pow(a_enc, b, ek.nn) * (1 + bp * ek.n) * pow(r, ek.n, ek.nn) % ek.nn) + items[k][2:]
    items[1] = (items[1][0] + items[1][4].nn,) + items[1][1:]   # an unreduced a_enc
    ctx, rng = PowContext(), LoggedRng("bob-prover-fused-draws")
    got = mta.generate_bob(items, rng, ctx=ctx, check=check, fused=True)
    # the draws and their order are the composed prover's (and the reference's)
    replay, per = LoggedRng("bob-prover-fused-draws"), []
    for it in items:
        N, Nt = it[4].n, it[5].N
        alpha = replay.sample_below(Q3)
        beta = replay.sample_below(N)
        while math.gcd(beta, N) != 1:    # from_modulo
            beta = replay.sample_below(N)
        per.append([alpha, beta] + [replay.sample_below(b) for b in (Q * Q * N, Q * Nt, Q3 * Nt, Q * Nt, Q3 * Nt)])
    assert rng.bounds == replay.bounds and rng.values == replay.values
    # ONE pedersen_commit call: four instances per proof in the order z, z', t, w
    (pc,) = _calls(ctx, "pedersen_commit")
    assert pc["nl"] == 64 and pc["xl"] == 16 + 64 and pc["yl"] == 24 + 64 == mta.commit_yl(64)
    assert pc["xs"] == [x for it, d in zip(items, per) for x in (it[2], d[0], it[3], d[2])]
    assert pc["ys"] == [y for d in per for y in (d[3], d[4], d[5], d[6])]
    sts = [small_keys[0]["st"], small_keys[1]["st"]]
    assert pc["keys"] == [(s.N, s.g % s.N, s.ni % s.N) for s in sts]           # deduplicated
    assert pc["key_idx"] == [k % 2 for k in range(5) for _ in range(4)]
    # ONE bob_commit_v call: a_enc mod N^2, alpha, gamma mod N, beta
    (bv,) = _calls(ctx, "bob_commit_v")
    assert bv["nl"] == 64 and bv["fused"] is True
    assert bv["a_encs"] == [it[0] % it[4].nn for it in items] and bv["a_encs"][1] != items[1][0]
    assert bv["alphas"] == [d[0] for d in per] and bv["betas"] == [d[1] for d in per]
    assert bv["gammas"] == [d[2] % it[4].n for it, d in zip(items, per)]
    assert any(d[2] >= it[4].n for it, d in zip(items, per))                 # the reduction did something
    assert bv["ns"] == [small_keys[0]["ek"].n, small_keys[1]["ek"].n] and bv["n_idx"] == [0, 1, 0, 1, 0]
    # no regular-access modexp; r^e alone goes through modexp_batch
    assert _calls(ctx, "modexp_batch") == [dict(count=5, nl=64, secret=False)]
    assert (len(_calls(ctx, "ec_mul_g")) == 1) == check
    # the oracle's prover under the same stream, and the composed path, field by field
    orng = Rng("bob-prover-fused-draws")
    for g, it in zip(got, items):
        pf, u = mo.generate(*it, orng, check=check)
        inner = g.proof if check else g
        assert [getattr(inner, f) for f in mo.FIELDS] == [getattr(pf, f) for f in mo.FIELDS]
        if check:
            assert g.u == u
    cctx = PowContext()
    assert mta.generate_bob(items, Rng("bob-prover-fused-draws"), ctx=cctx, check=check) == got
    assert [c["secret"] for c in _calls(cctx, "modexp_batch")] == [True, True, False, False]
    X = [ec.mul(ec.G, it[2]) for it in items] if check else [None] * 5
    assert [mo.outcome(p, it[0], it[1], it[4], it[5], x) for p, it, x in zip(got, items, X)] == [1] * 5


def test_generate_bob_fused_width_class_and_errors(small_keys):
    from fsdkr import mta
    from fsdkr.types import DLogStatement
    items = _items(small_keys, 2, "bob-prover-fused-wide")
    wide = DLogStatement((1 << 2100) + 1, 3, 5)            # an N~ above 2048 bits: the 3072-bit class
    ctx = PowContext()
    mta.generate_bob([items[0], items[1][:5] + (wide,) + items[1][6:]], Rng("w"), ctx=ctx, fused=True)
    (pc,) = _calls(ctx, "pedersen_commit")
    (bv,) = _calls(ctx, "bob_commit_v")
    assert (pc["nl"], pc["xl"], pc["yl"], bv["nl"]) == (96, 112, 120, 96)
    N = items[1][4].n
    for col, bad in ((2, -1), (2, 1 << 256), (3, -1), (3, N)):
        ctx, rng = PowContext(), LoggedRng("w")
        broken = items[1][:col] + (bad,) + items[1][col + 1:]
        with pytest.raises(ValueError):
            mta.generate_bob([items[0], broken], rng, ctx=ctx, fused=True)
        assert ctx.calls == [] and rng.bounds == []        # before any device call and any draw
    assert mta.generate_bob([], Rng("w"), ctx=PowContext(), fused=True) == []
    # the composed prover keeps taking such a beta' (no new refusal without the flag)
    mta.generate_bob([items[1][:3] + (N,) + items[1][4:]], Rng("w"), ctx=PowContext())


@pytest.mark.parametrize("check", [False, True])
def test_respond_passes_the_flag_on(small_keys, check):
    from fsdkr import mta
    rng = Rng("bob-prover-fused-respond")
    keys = [small_keys[k % 2] for k in range(3)]
    a_encs = [paillier.encrypt(k["ek"], rng.sample_below(Q), rng) for k in keys]
    bs = [rng.sample_below(Q) for _ in keys]
    eks, sts = [k["ek"] for k in keys], [k["st"] for k in keys]
    plain, fctx = PowContext(), PowContext()
    want = mta.respond(a_encs, bs, eks, sts, Rng("draws"), ctx=plain, check=check)
    got = mta.respond(a_encs, bs, eks, sts, Rng("draws"), ctx=fctx, check=check, fused_proofs=True)
    assert got == want
    assert _calls(plain, "pedersen_commit") == [] and _calls(plain, "bob_commit_v") == []
    assert len(_calls(fctx, "pedersen_commit")) == 1 and len(_calls(fctx, "bob_commit_v")) == 1
    assert [c["secret"] for c in _calls(fctx, "modexp_batch")] == [False]


# ---- the tail's schedule (csrc/mta_ct.hip bob_v_tail_ct_kernel) --------------------
LO = 768


def head_model(beta, N, w, NN):
    """modexp_slide_kernel's head over N's bits >= 768: sliding windows of at most w
    bits that never reach below bit 768; a head without such a bit hands over 1.
    Returns (state, odd-power table)."""
    T = [pow(beta, 2 * k + 1, NN) for k in range(1 << (w - 1))]
    x, i, first = 1, N.bit_length() - 1, True
    while i >= LO:
        if not (N >> i) & 1:
            x, i = x * x % NN, i - 1
            continue
        j = max(i - w + 1, LO)
        while not (N >> j) & 1:
            j += 1
        d = (N >> j) & ((1 << (i - j + 1)) - 1)
        if first:
            x = T[d >> 1]
        else:
            for _ in range(i - j + 1):
                x = x * x % NN
            x = x * T[d >> 1] % NN
        first, i = False, j - 1
    return x, T


def tail_model(x, T, N, a_enc, alpha, w, NN):
    """The kernel's 768 squarings from the head's state and table: N's low 768 bits
    leave from the top of a 24-limb shift register, a sliding window (a set bit down
    to its lowest set bit, at most w bits) multiplies its odd power in after its last
    squaring; alpha is read one 32-bit limb at a time, top limb first, and after every
    4th squaring the limb's top digit multiplies T2[digit] in, T2[0] = 1 included.
    Returns (value, window products, digit products, limbs read)."""
    T2 = [pow(a_enc, u, NN) for u in range(16)]
    M = (1 << LO) - 1
    nw = N & M
    limbs = [(alpha >> (32 * k)) & 0xFFFFFFFF for k in range(24)]
    pend = pend_d = 0
    n_win = n_dig = 0
    read = []
    for k in range(23, -1, -1):
        aw = limbs[k]
        read.append(k)
        for _ in range(8):
            for _ in range(4):
                if pend == 0 and nw >> (LO - 1):
                    top = nw >> (LO - w)
                    tz = (top & -top).bit_length() - 1
                    pend_d, pend = top >> tz, w - tz
                nw = (nw << 1) & M
                x = x * x % NN
                if pend:
                    pend -= 1
                    if pend == 0:
                        x = x * T[pend_d >> 1] % NN
                        n_win += 1
            nib, aw = aw >> 28, (aw << 4) & 0xFFFFFFFF
            x = x * T2[nib] % NN
            n_dig += 1
        assert aw == 0
    assert pend == 0 and nw == 0
    return x, n_win, n_dig, read


def _model_moduli(rng):
    ones, low = (1 << LO) - 1, 1
    out = []
    for bits in (600, 768, 769, 1100):
        out.append(rng.bits(bits) | (1 << (bits - 1)) | 1)
    out.append((rng.bits(1100) | (1 << 1099)) | ones)                  # low 768 bits all ones
    out.append(((rng.bits(1100) | (1 << 1099)) >> LO << LO) | low)     # low 768 bits zero but bit 0
    out.append((1 << LO) - 1)                                          # exactly 768 bits, all ones
    return out


@pytest.mark.parametrize("w", [5, 6, 7])
def test_tail_schedule_model(w):
    rng = Rng(("bob-v-tail-model", w))
    alt = int("0f" * 96, 16)
    edge = [0, 1, 15, 16, 1 << 256, 1 << 767, 0xF << 764, (1 << 768) - 1, Q3 - 1, alt, 0xDEADBEEF << (32 * 8),
            0x80000001 << (32 * 23), rng.bits(768)]
    for t, N in enumerate(_model_moduli(rng)):
        NN = N * N
        beta = rng.sample_below(N)
        x, T = head_model(beta, N, w, NN)
        assert x == pow(beta, N >> LO, NN)
        wins = set()
        for q, alpha in enumerate(edge):
            a_enc = [rng.sample_below(NN), 0, 1, N, NN - 1][(t + q) % 5]
            got, n_win, n_dig, read = tail_model(x, T, N, a_enc, alpha, w, NN)
            assert got == pow(beta, N, NN) * pow(a_enc, alpha, NN) % NN
            assert n_dig == 192                             # every digit, zero digits as well, for every alpha
            assert read == list(range(23, -1, -1))          # one limb at a time, whatever alpha
            wins.add(n_win)
        assert len(wins) == 1                               # the window schedule is N's alone
