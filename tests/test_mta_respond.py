"""CPU checks of Bob's MtA response: fsdkr.mta.respond / finish over a stand-in
context that serves the device calls with pow (draw order, width class, the
reduction of a_enc, the ValueErrors, beta = -beta' mod q); a Python model of the
constant-time tail's schedule (csrc/mta_ct.hip) against pow; and the wire
encoding of BobProof / BobProofExt."""
import json

import pytest

import mta_oracle as mo
from oracle import paillier
from oracle import secp256k1 as ec
from oracle.rng import Rng

Q = ec.Q


# ---- a stand-in context: the device calls by pow, recorded -------------------------
class PowContext:
    def __init__(self):
        self.calls = []

    def mta_respond(self, a_encs, bs, beta_prims, rs, ns, n_idx, nl, fused=True):
        self.calls.append(("mta_respond", dict(a_encs=list(a_encs), bs=list(bs), beta_prims=list(beta_prims),
                                               rs=list(rs), ns=list(ns), n_idx=list(n_idx), nl=nl, fused=fused)))
        out = []
        for a, b, bp, r, i in zip(a_encs, bs, beta_prims, rs, n_idx):
            N = ns[i]
            assert 0 <= a < N * N
            out.append(pow(a, b, N * N) * (1 + bp * N) * pow(r, N, N * N) % (N * N))
        return out

    def modexp_batch(self, bases, exps, mods, mod_idx, mod_limbs, secret=False):
        self.calls.append(("modexp_batch", dict(count=len(bases), nl=mod_limbs, secret=secret)))
        return [pow(b, e, mods[i]) for b, e, i in zip(bases, exps, mod_idx)]

    def ec_mul_g(self, scalars):
        self.calls.append(("ec_mul_g", dict(count=len(scalars))))
        return [ec.mul(ec.G, s) for s in scalars]

    def paillier_decrypt(self, cts, p, q, nl):
        self.calls.append(("paillier_decrypt", dict(count=len(cts), nl=nl)))
        return [paillier.decrypt(paillier.DecryptionKey(p, q), c) for c in cts]

    def paillier_decrypt_many(self, cts, key_idx, ps, qs, nl):
        self.calls.append(("paillier_decrypt_many", dict(count=len(cts), nl=nl)))
        return [paillier.decrypt(paillier.DecryptionKey(ps[i], qs[i]), c) for c, i in zip(cts, key_idx)]


class LoggedRng:
    def __init__(self, seed):
        self.rng, self.bounds = Rng(seed), []

    def sample_below(self, upper):
        self.bounds.append(upper)
        return self.rng.sample_below(upper)


@pytest.fixture(scope="module")
def small_keys():
    """Two 768-bit Paillier keys with a statement each (the 2048-bit class; a b < 2^512
    for every b below 2^256, so a b + beta' wraps N at most once)."""
    rng = Rng("mta-respond-cpu-keys")
    out = []
    for _ in range(2):
        ek, dk = paillier.keypair_with_modulus_size(768, rng)
        ekt, dkt = paillier.keypair_with_modulus_size(768, rng)
        out.append(dict(ek=ek, dk=dk, st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)))
    return out


def _exchange(small_keys, n, seed):
    rng = Rng(seed)
    keys = [small_keys[k % 2] for k in range(n)]
    a = [rng.sample_below(Q) for _ in keys]
    a_encs = [paillier.encrypt(k["ek"], x, rng) for k, x in zip(keys, a)]
    bs = [rng.sample_below(Q) for _ in keys]
    return keys, a, a_encs, bs


@pytest.mark.parametrize("check", [False, True])
def test_respond_and_finish_over_pow(small_keys, check):
    from fsdkr import mta
    keys, a, a_encs, bs = _exchange(small_keys, 5, "mta-respond-cpu")
    eks, sts = [k["ek"] for k in keys], [k["st"] for k in keys]
    # any value below 2^256 (b = 0 in the plain proof only: with check X = G*0 is the
    # point at infinity and the reference's prover panics on its coordinates)
    bs[1], bs[2] = (1 if check else 0), (1 << 256) - 1
    given = [c + (k % 2) * ek.nn for k, (c, ek) in enumerate(zip(a_encs, eks))]   # some unreduced
    ctx, rng = PowContext(), LoggedRng("mta-respond-cpu-draws")
    mta_outs, betas, proofs = mta.respond(given, bs, eks, sts, rng, ctx=ctx, check=check)
    # draw order: per item beta' then r, both below N, before any draw of the proofs
    assert rng.bounds[:10] == [ek.n for ek in eks for _ in range(2)]
    assert rng.bounds[10] == Q ** 3                        # generate_bob's alpha follows
    replay = Rng("mta-respond-cpu-draws")
    draws = [(replay.sample_below(ek.n), replay.sample_below(ek.n)) for ek in eks]
    assert betas == [(-bp) % Q for bp, _ in draws]
    # ONE mta_respond call: reduced a_enc, deduplicated keys, the 2048-bit class
    name, call = ctx.calls[0]
    assert name == "mta_respond" and [c[0] for c in ctx.calls].count("mta_respond") == 1
    assert call["a_encs"] == a_encs and call["bs"] == bs and call["nl"] == 64 and call["fused"] is True
    assert call["beta_prims"] == [d[0] for d in draws] and call["rs"] == [d[1] for d in draws]
    assert call["ns"] == [small_keys[0]["ek"].n, small_keys[1]["ek"].n] and call["n_idx"] == [0, 1, 0, 1, 0]
    want = [paillier.add(ek, paillier.mul(ek, c, b), paillier.encrypt_with_chosen_randomness(ek, bp, r))
            for ek, c, b, (bp, r) in zip(eks, a_encs, bs, draws)]
    assert mta_outs == want
    # the proofs are generate_bob's over the same stream, on the values as given
    items = [(c, m, b, bp, ek, st, r) for c, m, b, (bp, r), ek, st in zip(given, mta_outs, bs, draws, eks, sts)]
    assert proofs == mta.generate_bob(items, replay, ctx=PowContext(), check=check)
    assert ("ec_mul_g" in [c[0] for c in ctx.calls]) == check
    X = [ec.mul(ec.G, b) for b in bs] if check else [None] * 5
    assert [mo.outcome(p, c, m, ek, st, x) for p, c, m, ek, st, x in zip(proofs, given, mta_outs, eks, sts, X)] == [1] * 5
    # Alice's last step
    fctx = PowContext()
    alphas = mta.finish(mta_outs, [k["dk"] for k in keys], ctx=fctx)
    assert [c[0] for c in fctx.calls] == ["paillier_decrypt_many"] and fctx.calls[0][1]["nl"] == 64
    assert [(al + be) % Q for al, be in zip(alphas, betas)] == [x * b % Q for x, b in zip(a, bs)]
    fctx = PowContext()
    assert mta.finish(mta_outs[::2], [keys[0]["dk"]] * 3, ctx=fctx) == alphas[::2]
    assert [c[0] for c in fctx.calls] == ["paillier_decrypt"]


def test_respond_width_class_and_errors(small_keys):
    from fsdkr import mta
    from fsdkr.types import DLogStatement
    keys, a, a_encs, bs = _exchange(small_keys, 2, "mta-respond-cpu-wide")
    eks = [k["ek"] for k in keys]
    wide = DLogStatement((1 << 2100) + 1, 3, 5)            # an N~ above 2048 bits: the 3072-bit class
    ctx = PowContext()
    mta.respond(a_encs, bs, eks, [keys[0]["st"], wide], Rng("w"), ctx=ctx)
    assert ctx.calls[0][1]["nl"] == 96
    assert all(c[1]["nl"] in (96, 192) for c in ctx.calls if c[0] == "modexp_batch")
    sts = [k["st"] for k in keys]
    for bad in (-1, 1 << 256):
        ctx = PowContext()
        with pytest.raises(ValueError):
            mta.respond(a_encs, [bs[0], bad], eks, sts, Rng("w"), ctx=ctx)
        assert ctx.calls == []
    with pytest.raises(ValueError):
        mta.respond(a_encs, bs[:1], eks, sts, Rng("w"), ctx=PowContext())
    assert mta.respond([], [], [], [], Rng("w"), ctx=PowContext()) == ([], [], [])
    assert mta.finish([], [], ctx=PowContext()) == []


# ---- the tail's schedule (csrc/mta_ct.hip mta_tail_ct_kernel) ----------------------
def tail_model(x, T, N, a_enc, b, w, NN):
    """The kernel's 256 squarings from the head's state x = r^(N >> 256) and its
    odd-power table T[k] = r^(2k + 1): N's low 256 bits leave from the top of a
    shift register, a sliding window (a set bit down to its lowest set bit, at most w
    bits) multiplies its odd power in after its last squaring, and after every 4th
    squaring b's digit multiplies T2[digit] in, T2[0] = 1 included.  Returns
    (value, window products, digit products)."""
    T2 = [pow(a_enc, u, NN) for u in range(16)]
    nw, bw = N & ((1 << 256) - 1), b
    pend = pend_d = 0
    n_win = n_dig = 0
    for _ in range(64):
        for _ in range(4):
            if pend == 0 and nw >> 255:
                top = nw >> (256 - w)
                tz = (top & -top).bit_length() - 1
                pend_d, pend = top >> tz, w - tz
            nw = (nw << 1) & ((1 << 256) - 1)
            x = x * x % NN
            if pend:
                pend -= 1
                if pend == 0:
                    x = x * T[pend_d >> 1] % NN
                    n_win += 1
        nib, bw = bw >> 252, (bw << 4) & ((1 << 256) - 1)
        x = x * T2[nib] % NN
        n_dig += 1
    assert pend == 0 and nw == 0 and bw == 0
    return x, n_win, n_dig


@pytest.mark.parametrize("w", [5, 6, 7])
def test_tail_schedule_model(w):
    rng = Rng(("mta-tail-model", w))
    alt = int("0f" * 32, 16)
    edge_b = [0, 1, 15, 16, Q - 1, (1 << 256) - 1, 0xF << 252, alt, rng.bits(256)]
    for t, N in enumerate([rng.bits(600) | (1 << 599) | 1, (1 << 600) + 1, (1 << 600) - 1,
                           rng.bits(600) | (1 << 599) | ((1 << 256) - 1)]):
        NN = N * N
        r = rng.sample_below(N)
        x = pow(r, N >> 256, NN)
        T = [pow(r, 2 * k + 1, NN) for k in range(1 << (w - 1))]
        wins = set()
        for b in edge_b:
            a_enc = [rng.sample_below(NN), 0, 1, N][(t + b) % 4]
            got, n_win, n_dig = tail_model(x, T, N, a_enc, b, w, NN)
            assert got == pow(r, N, NN) * pow(a_enc, b, NN) % NN
            assert n_dig == 64                              # zero digits are multiplied in as well
            wins.add(n_win)
        assert len(wins) == 1                               # the window schedule is N's alone


# ---- wire ----------------------------------------------------------------------
def test_wire_bob_proofs():
    from fsdkr import wire
    from fsdkr.types import BobProof, BobProofExt
    rng = Rng("mta-wire")
    pf = BobProof(*(rng.bits(64 + 50 * k) for k in range(8)))
    obj = wire.bob_proof_to_obj(pf)
    assert list(obj) == ["t", "z", "e", "s", "s1", "s2", "t1", "t2", "_phantom"]
    assert obj["_phantom"] is None and obj["t"] == format(pf.t, "x")
    text = wire.dumps(pf)
    assert text.endswith(',"_phantom":null}') and list(json.loads(text)) == list(obj)
    assert wire.loads(text, "BobProof") == pf
    for u in (ec.mul(ec.G, 7), ec.mul(ec.G, rng.sample_below(Q)), None):
        px = BobProofExt(pf, u)
        ox = wire.bob_proof_ext_to_obj(px)
        assert list(ox) == ["proof", "u"] and ox["proof"] == obj
        assert ox["u"]["curve"] == "secp256k1" and (ox["u"]["point"] == "00") == (u is None)
        assert wire.loads(wire.dumps(px), "BobProofExt") == px
