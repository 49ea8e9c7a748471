"""GPU checks of Alice's side of MtA (fsdkr.mta.initiate / generate_alice /
verify_alice, fsdkr_alice_verify, fsdkr_pedersen_commit_ct): the first message and
its proofs bit for bit against oracle.paillier and oracle.range_proofs under the
same seeded stream, in both width classes; the verifier's verdicts against the
oracle's on honest and tampered proofs with the keys mixed in one call; and the
whole exchange initiate -> verify_alice -> respond -> verify_bob -> finish."""
import dataclasses

import pytest

import mta_oracle as mo
from oracle import paillier
from oracle import range_proofs as rp
from oracle import secp256k1 as ec
from oracle.paillier import EncryptionKey
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

Q = ec.Q
Q3 = Q ** 3


def _key_sets(ctx, rng, bits, sets):
    from fsdkr import keygen
    kps = keygen.keypairs_with_modulus_size(ctx, rng, bits, 2 * sets)
    out = []
    for k in range(sets):
        ek, dk = kps[2 * k]
        ekt, dkt = kps[2 * k + 1]
        out.append(dict(ek=EncryptionKey.from_n(ek.n), dk=dk, st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng), pt=dkt.p))
    return out


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    """Two key sets of 2048 bits and one of 3072 (a Paillier key and an N~ each,
    device-generated); pt is a prime factor of N~."""
    rng = Rng("mta-alice-keys")
    return dict(k2048=_key_sets(gpu_ctx, rng, 2048, 2), k3072=_key_sets(gpu_ctx, rng, 3072, 1))


def _t(pf):
    return dataclasses.astuple(pf)


def _oracle(ks, as_, seed):
    """The reference's alice_zkp (:650-670) per exchange over one stream in initiate's
    order: every r first, then the proofs."""
    rng = Rng(seed)
    rs = [rng.from_modulo(k["ek"].n) for k in ks]
    cs = [paillier.encrypt_with_chosen_randomness(k["ek"], a, r) for k, a, r in zip(ks, as_, rs)]
    return cs, rs, [rp.generate(a, c, k["ek"], k["st"], r, rng) for k, a, c, r in zip(ks, as_, cs, rs)]


@pytest.fixture(scope="module")
def exchanges(gpu_ctx, keys):
    """6 exchanges over the two 2048-bit key sets and 3 over the 3072-bit set, each
    class one initiate call; with the oracle's values under the same seed."""
    from fsdkr import mta
    out = {}
    for tag, ks in (("nl64", [keys["k2048"][k % 2] for k in range(6)]), ("nl96", [keys["k3072"][0]] * 3)):
        rng = Rng(("mta-alice-a", tag))
        as_ = [0, Q - 1] + [rng.sample_below(Q) for _ in range(len(ks) - 2)]
        eks, sts = [k["ek"] for k in ks], [k["st"] for k in ks]
        got = mta.initiate(as_, eks, sts, Rng(("mta-alice", tag)), ctx=gpu_ctx)
        out[tag] = dict(ks=ks, as_=as_, eks=eks, sts=sts, got=got, want=_oracle(ks, as_, ("mta-alice", tag)))
    return out


@pytest.mark.parametrize("tag", ["nl64", "nl96"])
def test_initiate_matches_the_oracle(exchanges, tag):
    x = exchanges[tag]
    a_encs, rs, proofs = x["got"]
    want_c, want_r, want_p = x["want"]
    assert a_encs == want_c and rs == want_r
    assert [_t(p) for p in proofs] == [_t(p) for p in want_p]


def _oracle_verdict(pf, c, ek, st):
    return int(rp.verify(rp.AliceProof(*_t(pf)), c, ek, st))


@pytest.mark.parametrize("tag", ["nl64", "nl96"])
def test_verify_accepts(gpu_ctx, exchanges, tag):
    from fsdkr import mta
    x = exchanges[tag]
    a_encs, _, proofs = x["got"]
    assert list(mta.verify_alice(proofs, a_encs, x["eks"], x["sts"], ctx=gpu_ctx)) == [1] * len(proofs)
    assert [_oracle_verdict(p, c, ek, st) for p, c, ek, st in zip(proofs, a_encs, x["eks"], x["sts"])] == [1] * len(proofs)


def _tampered(exchanges):
    """(proof, cipher, key set) rows: one tamper per field, the s1 bound on both sides,
    the non-units, the challenge's edge values; the 2048- and 3072-bit keys alternate."""
    rows = []
    pool = []
    for tag in ("nl64", "nl96"):
        x = exchanges[tag]
        pool.append([(p, c, k) for p, c, k in zip(x["got"][2], x["got"][0], x["ks"])])
    kinds = ["z", "e", "s", "s1", "s2", "cipher", "s1=q3", "s1=q3+1", "z=0", "z|p", "cipher|p", "e=0", "e=2^256",
             "honest", "z", "cipher|p", "s1=q3+1", "e=2^256"]
    for i, kind in enumerate(kinds):
        src = pool[i % 2]
        pf, c, k = src[(i // 2) % len(src)]
        N, Nt = k["ek"].n, k["st"].N
        if kind in ("z", "e", "s", "s1", "s2"):
            pf = dataclasses.replace(pf, **{kind: getattr(pf, kind) + 1})
        elif kind == "cipher":
            c = c + 1
        elif kind == "s1=q3":
            pf = dataclasses.replace(pf, s1=Q3)
        elif kind == "s1=q3+1":
            pf = dataclasses.replace(pf, s1=Q3 + 1)
        elif kind == "z=0":
            pf = dataclasses.replace(pf, z=0)
        elif kind == "z|p":
            pf = dataclasses.replace(pf, z=pf.z * k["pt"] % Nt)
        elif kind == "cipher|p":
            c = c * k["dk"].p % (N * N)
        elif kind == "e=0":
            pf = dataclasses.replace(pf, e=0)
        elif kind == "e=2^256":
            pf = dataclasses.replace(pf, e=1 << 256)
        rows.append((kind, pf, c, k))
    return rows


def test_verify_rejects_as_the_oracle(gpu_ctx, exchanges):
    from fsdkr import mta
    from fsdkr.batch import UnsupportedInput
    rows = _tampered(exchanges)
    assert len(rows) >= 14
    pfs, cs = [r[1] for r in rows], [r[2] for r in rows]
    eks, sts = [r[3]["ek"] for r in rows], [r[3]["st"] for r in rows]
    want = [_oracle_verdict(p, c, ek, st) for p, c, ek, st in zip(pfs, cs, eks, sts)]
    assert want == [1 if r[0] == "honest" else 0 for r in rows]
    # the keys mixed in one call (the 3072-bit class, the 2048-bit keys zero-extended)
    assert list(mta.verify_alice(pfs, cs, eks, sts, ctx=gpu_ctx)) == want
    # the 2048-bit rows alone: the 64-limb class
    sub = [i for i, r in enumerate(rows) if r[3]["ek"].n.bit_length() <= 2048]
    assert len(sub) >= 7
    got = mta.verify_alice([pfs[i] for i in sub], [cs[i] for i in sub], [eks[i] for i in sub], [sts[i] for i in sub],
                           ctx=gpu_ctx)
    assert list(got) == [want[i] for i in sub]
    # s >= N^2 has no place in its field
    k = rows[0][3]
    with pytest.raises(UnsupportedInput):
        mta.verify_alice([dataclasses.replace(rows[0][1], s=k["ek"].n ** 2)], cs[:1], eks[:1], sts[:1], ctx=gpu_ctx)


def test_verify_error_returns(gpu_ctx, exchanges):
    from fsdkr import _native, mta
    x = exchanges["nl64"]
    a_encs, _, proofs = x["got"]
    pp = mta.prepass_alice(proofs, a_encs, x["eks"], x["sts"])
    b, keep = mta._alice_batch(pp, a_encs, proofs)
    b.nl = 80
    with pytest.raises(_native.FsdkrError) as e:
        gpu_ctx.alice_verify(b, pp["count"])
    assert e.value.code == _native.FSDKR_E_UNSUPPORTED
    b.nl = 64
    try:
        gpu_ctx.set_modexp_group(2)
        with pytest.raises(_native.FsdkrError) as e:
            gpu_ctx.alice_verify(b, pp["count"])
        assert e.value.code == _native.FSDKR_E_ARG
        for lanes in (4, 8):
            gpu_ctx.set_modexp_group(lanes)
            assert list(gpu_ctx.alice_verify(b, pp["count"])) == [1] * pp["count"]
    finally:
        gpu_ctx.set_modexp_group(0)
    assert list(gpu_ctx.alice_verify(b, 0)) == []


def test_whole_exchange(gpu_ctx, exchanges):
    """initiate -> verify_alice -> respond -> verify_bob -> finish: alpha + beta = a b mod q."""
    from fsdkr import mta
    x = exchanges["nl64"]
    a_encs, _, proofs = x["got"]
    eks, sts = x["eks"], x["sts"]
    assert list(mta.verify_alice(proofs, a_encs, eks, sts, ctx=gpu_ctx)) == [1] * 6
    rng = Rng("mta-alice-whole")
    bs = [rng.sample_below(Q) for _ in range(6)]
    mta_outs, betas, bob = mta.respond(a_encs, bs, eks, sts, rng, ctx=gpu_ctx)
    assert list(mta.verify_bob(bob, a_encs, mta_outs, eks, sts, ctx=gpu_ctx)) == [1] * 6
    alphas = mta.finish(mta_outs, [k["dk"] for k in x["ks"]], ctx=gpu_ctx)
    assert [(al + be) % Q for al, be in zip(alphas, betas)] == [a * b % Q for a, b in zip(x["as_"], bs)]
