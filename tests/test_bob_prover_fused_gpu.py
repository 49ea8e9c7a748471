"""GPU checks of Bob's prover on the constant-time entries
(fsdkr.mta.generate_bob(fused=True), respond(fused_proofs=True)): the proofs equal
the oracle's prover field by field under the same seeded stream and the composed
prover's bit for bit, both verifiers accept them, and a recording context shows one
pedersen_commit call of 4 n instances at the public widths, one bob_commit_v call
and no regular-access modexp.  Keys: the golden 1024-bit key, two device-generated
2048-bit key sets mixed in one call, and a 3072-bit key set (the composed v with the
comb at 112 / 120 limbs)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import codec  # noqa: E402
import mta_oracle as mo  # noqa: E402
from oracle import secp256k1 as ec  # noqa: E402
from oracle.paillier import EncryptionKey  # noqa: E402
from oracle.rng import Rng  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec_ctx():
    """A context of its own that records the calls the prover issues."""
    from fsdkr import Context

    class Recorder(Context):
        def __init__(self):
            super().__init__()
            self.calls = []

        def pedersen_commit(self, xs, ys, keys, key_idx, nl, xl=None, yl=None):
            self.calls.append(("pedersen_commit", dict(count=len(xs), nl=nl, xl=xl, yl=yl)))
            return super().pedersen_commit(xs, ys, keys, key_idx, nl, xl=xl, yl=yl)

        def bob_commit_v(self, a_encs, alphas, gammas, betas, ns, n_idx, nl, fused=True):
            self.calls.append(("bob_commit_v", dict(count=len(a_encs), nl=nl, fused=fused)))
            return super().bob_commit_v(a_encs, alphas, gammas, betas, ns, n_idx, nl, fused=fused)

        def modexp_batch(self, bases, exps, mods, mod_idx, mod_limbs, secret=False):
            self.calls.append(("modexp_batch", dict(count=len(bases), secret=bool(secret))))
            return super().modexp_batch(bases, exps, mods, mod_idx, mod_limbs, secret=secret)

    ctx = Recorder()
    yield ctx
    ctx.close()


def _key_sets(ctx, rng, bits, sets):
    from fsdkr import keygen
    kps = keygen.keypairs_with_modulus_size(ctx, rng, bits, 2 * sets)
    out = []
    for k in range(sets):
        ek, dk = kps[2 * k]
        ekt, dkt = kps[2 * k + 1]
        out.append(dict(ek=EncryptionKey.from_n(ek.n), st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)))
    return out


@pytest.fixture(scope="module")
def sets64(rec_ctx):
    """The golden 1024-bit key (its first Paillier key, its second statement) between
    two device-generated 2048-bit key sets."""
    raw = codec.load_raw("transcript_join_t1_n4_kb1024.json.gz")
    assert raw["meta"]["key_bits"] == 1024
    gk = codec.dec(raw["keys"], codec.product_classes())[0]
    golden = dict(ek=EncryptionKey.from_n(gk.paillier_key_vec[0].n), st=gk.h1_h2_n_tilde_vec[1])
    a, b = _key_sets(rec_ctx, Rng("bob-prover-fused-keys"), 2048, 2)
    return [a, golden, b]


@pytest.fixture(scope="module")
def sets96(rec_ctx):
    return _key_sets(rec_ctx, Rng("bob-prover-fused-keys-96"), 3072, 1)


def _items(sets, n, seed):
    items = []
    for k in range(n):
        key = sets[k % len(sets)]
        a_enc, m, b, beta_prim, r = mo.mta_scenario(key["ek"], Rng((seed, k)))
        items.append((a_enc, m, b, beta_prim, key["ek"], key["st"], r))
    return items


def _check_prover(ctx, items, nl, check, seed):
    from fsdkr import mta
    n = len(items)
    ctx.calls.clear()
    got = mta.generate_bob(items, Rng(seed), ctx=ctx, check=check, fused=True)
    calls = list(ctx.calls)
    # one comb call of 4 n instances at the public widths, one v call, no secret modexp
    assert [c[1] for c in calls if c[0] == "pedersen_commit"] == [dict(count=4 * n, nl=nl, xl=16 + nl, yl=24 + nl)]
    assert [c[1] for c in calls if c[0] == "bob_commit_v"] == [dict(count=n, nl=nl, fused=True)]
    assert [c[1] for c in calls if c[0] == "modexp_batch"] == [dict(count=n, secret=False)]
    # the oracle's prover under the same stream, field by field
    orng = Rng(seed)
    for g, it in zip(got, items):
        pf, u = mo.generate(*it, orng, check=check)
        inner = g.proof if check else g
        assert [getattr(inner, f) for f in mo.FIELDS] == [getattr(pf, f) for f in mo.FIELDS]
        if check:
            assert g.u == u
    # the composed prover, bit for bit
    ctx.calls.clear()
    assert mta.generate_bob(items, Rng(seed), ctx=ctx, check=check) == got
    assert [c[1]["secret"] for c in ctx.calls if c[0] == "modexp_batch"] == [True, True, False, False]
    # both verifiers accept
    a_encs, mtas = [it[0] for it in items], [it[1] for it in items]
    eks, sts = [it[4] for it in items], [it[5] for it in items]
    X = [ec.mul(ec.G, it[2]) for it in items] if check else None
    assert list(mta.verify_bob(got, a_encs, mtas, eks, sts, X=X, ctx=ctx)) == [1] * n
    assert [mo.outcome(p, a, m, ek, st, x) for p, a, m, ek, st, x in
            zip(got, a_encs, mtas, eks, sts, X or [None] * n)] == [1] * n


@pytest.mark.parametrize("check", [False, True])
def test_generate_bob_fused_2048(rec_ctx, sets64, check):
    _check_prover(rec_ctx, _items(sets64, 6, "bob-prover-fused-gpu"), 64, check, ("bob-prover-fused-draws", check))


@pytest.mark.parametrize("check", [False, True])
def test_generate_bob_fused_3072(rec_ctx, sets96, check):
    _check_prover(rec_ctx, _items(sets96, 2, "bob-prover-fused-gpu-96"), 96, check, ("bob-prover-fused-draws-96", check))


@pytest.mark.parametrize("check", [False, True])
def test_respond_fused_proofs(rec_ctx, sets64, check):
    from fsdkr import mta
    rng = Rng("bob-prover-fused-respond")
    keys = [sets64[k % 3] for k in range(4)]
    ns = sorted({k["ek"].n for k in keys})
    a_encs = rec_ctx.paillier_encrypt([rng.sample_below(ec.Q) for _ in keys], [rng.sample_below(k["ek"].n) for k in keys],
                                      ns, [ns.index(k["ek"].n) for k in keys], 64)
    bs = [rng.sample_below(ec.Q) for _ in keys]
    eks, sts = [k["ek"] for k in keys], [k["st"] for k in keys]
    want = mta.respond(a_encs, bs, eks, sts, Rng("draws"), ctx=rec_ctx, check=check)
    rec_ctx.calls.clear()
    got = mta.respond(a_encs, bs, eks, sts, Rng("draws"), ctx=rec_ctx, check=check, fused_proofs=True)
    assert got == want
    assert [c[0] for c in rec_ctx.calls].count("pedersen_commit") == 1
    assert [c[0] for c in rec_ctx.calls].count("bob_commit_v") == 1
    assert not any(c[0] == "modexp_batch" and c[1]["secret"] for c in rec_ctx.calls)


def test_widest_b_and_beta_prim(rec_ctx, sets64):
    """b = 2^256 - 1 and beta' = N - 1 go through; b = 2^256 is refused before any device call."""
    from fsdkr import mta
    items = _items(sets64, 2, "bob-prover-fused-edges")
    for k, (col, v) in enumerate(((2, (1 << 256) - 1), (3, items[1][4].n - 1))):
        it = items[k][:col] + (v,) + items[k][col + 1:]
        a_enc, _, b, bp, ek, st, r = it
        items[k] = (a_enc, pow(a_enc, b, ek.nn) * (1 + bp * ek.n) * pow(r, ek.n, ek.nn) % ek.nn) + it[2:]
    got = mta.generate_bob(items, Rng("edges"), ctx=rec_ctx, fused=True)
    assert got == mta.generate_bob(items, Rng("edges"), ctx=rec_ctx)
    assert [mo.outcome(p, it[0], it[1], it[4], it[5]) for p, it in zip(got, items)] == [1, 1]
    rec_ctx.calls.clear()
    with pytest.raises(ValueError):
        mta.generate_bob([items[0][:2] + (1 << 256,) + items[0][3:]], Rng("edges"), ctx=rec_ctx, fused=True)
    assert rec_ctx.calls == []
