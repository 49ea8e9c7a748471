"""GPU checks of Bob's MtA response (fsdkr_mta_respond, fsdkr.mta.respond /
finish): the constant-time fused chain and the composed path against Python's
pow and oracle.paillier bit for bit, on edge values of every operand and on
counts around a wave (8 chains) and a block (32); the error returns; and the
reference's bob_zkp scenario (range_proofs.rs:672-745) end to end on the device."""
import pytest

import mta_oracle as mo
from oracle import paillier
from oracle import secp256k1 as ec
from oracle.paillier import EncryptionKey
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

Q = ec.Q
COUNTS_64 = (1, 7, 8, 9, 31, 32, 33, 70)
COUNTS_96 = (1, 5, 9)


def _key_sets(ctx, rng, bits, sets):
    from fsdkr import keygen
    kps = keygen.keypairs_with_modulus_size(ctx, rng, bits, 2 * sets)
    out = []
    for k in range(sets):
        ek, dk = kps[2 * k]
        ekt, dkt = kps[2 * k + 1]
        out.append(dict(ek=EncryptionKey.from_n(ek.n), dk=dk, st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)))
    return out


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    """Two key sets of 2048 bits (four device-generated keys: a Paillier key and an
    N~ each) and the moduli of the width tests: one 1024-bit N and two 3072-bit N."""
    from fsdkr import keygen
    rng = Rng("mta-respond-keys")
    sets = _key_sets(gpu_ctx, rng, 2048, 2)
    short = keygen.keypairs_with_modulus_size(gpu_ctx, rng, 1024, 1)[0][0].n
    wide = [ek.n for ek, _ in keygen.keypairs_with_modulus_size(gpu_ctx, rng, 3072, 2)]
    assert short.bit_length() <= 1024 and all(n.bit_length() > 2048 for n in wide)
    return dict(sets=sets, short=short, wide=wide)


def _instances(ns, count, tag):
    """`count` responses with the keys interleaved instance by instance and every
    operand cycling through its edge values (the cycles are offset against each other
    and against the keys).  Returns (a_enc, b, beta_prim, r, key) rows."""
    rng = Rng(("mta-respond", tag))
    alt = int("0f" * 32, 16)                     # every second nibble zero
    out = []
    for i in range(count):
        m = i % len(ns)
        N = ns[m]
        NN = N * N
        b = [0, 1, 15, 16, Q - 1, (1 << 256) - 1, 0xF << 252, alt, rng.bits(256)][(i + i // 9) % 9]
        a = [0, 1, NN - 1, N, rng.sample_below(NN)][(i + i // 5) % 5]
        r = [1, N - 1, rng.sample_below(N)][(i + i // 3) % 3]
        bp = [0, 1, N - 1, rng.sample_below(N)][(i + i // 4) % 4]
        out.append((a, b, bp, r, m))
    return out


def _want(ns, inst):
    out = []
    for a, b, bp, r, m in inst:
        N = ns[m]
        out.append(pow(a, b, N * N) * (1 + bp * N) * pow(r, N, N * N) % (N * N))
    return out


@pytest.fixture(scope="module")
def ref64(keys):
    """The 70 instances of the 2048-bit class over three interleaved keys (one of
    1024 bits: the head's bit count differs per key) and their values by pow;
    every count uses a prefix."""
    ns = [keys["sets"][0]["ek"].n, keys["short"], keys["sets"][1]["ek"].n]
    inst = _instances(ns, max(COUNTS_64), "nl64")
    want = _want(ns, inst)
    ek = EncryptionKey.from_n(ns[0])
    a, b, bp, r, _ = inst[0]   # the oracle's composition gives the same value
    assert paillier.add(ek, paillier.mul(ek, a, b), paillier.encrypt_with_chosen_randomness(ek, bp, r)) == want[0]
    return ns, inst, want


@pytest.fixture(scope="module")
def ref96(keys):
    """9 instances of the 3072-bit class: two 3072-bit keys and one 2048-bit key
    zero-extended into the call."""
    ns = [keys["wide"][0], keys["sets"][0]["ek"].n, keys["wide"][1]]
    inst = _instances(ns, max(COUNTS_96), "nl96")
    return ns, inst, _want(ns, inst)


def _run(ctx, ns, inst, nl, fused):
    A, B, BP, R, I = (list(x) for x in zip(*inst))
    return ctx.mta_respond(A, B, BP, R, ns, I, nl, fused=fused)


# ---- 1. nl = 64: the fused chain and the composed path against pow -----------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("count", COUNTS_64)
def test_respond_2048_matches_pow(gpu_ctx, ref64, count, fused):
    ns, inst, want = ref64
    assert _run(gpu_ctx, ns, inst[:count], 64, fused) == want[:count]


@pytest.mark.parametrize("count", [12289, 24577])
def test_respond_2048_head_shapes(gpu_ctx, ref64, count):
    """The fused chain's head picks its lanes as the keyed launches do: 16 up to 12288
    chains (every count above), 8 up to 24576, then 4 (16 chains per wave: a key's run
    is padded to whole waves of the head as well); the tail stays at 8.  The first 45
    instances (every edge combination once per key) repeated to `count`."""
    ns, inst, want = ref64
    k = [i % 45 for i in range(count)]
    assert _run(gpu_ctx, ns, [inst[i] for i in k], 64, True) == [want[i] for i in k]


# ---- 2. nl = 96 ------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("count", COUNTS_96)
def test_respond_3072_matches_pow(gpu_ctx, ref96, count, fused):
    ns, inst, want = ref96
    assert _run(gpu_ctx, ns, inst[:count], 96, fused) == want[:count]


# ---- 3. error returns --------------------------------------------------------------
def test_error_returns(gpu_ctx, ref64):
    from fsdkr import _native
    ns, inst, want = ref64
    with pytest.raises(_native.FsdkrError) as e:
        _run(gpu_ctx, ns, inst[:3], 80, True)
    assert e.value.code == _native.FSDKR_E_UNSUPPORTED
    for fused in (True, False):
        with pytest.raises(_native.FsdkrError) as e:
            _run(gpu_ctx, [ns[0], ns[1] + 1, ns[2]], [(1, 1, 1, 1, m) for m in range(3)], 64, fused)
        assert e.value.code == _native.FSDKR_E_ARG
        assert gpu_ctx.mta_respond([], [], [], [], ns, [], 64, fused=fused) == []
    # a_enc is public: an unreduced one is refused, not silently reduced
    with pytest.raises(_native.FsdkrError) as e:
        _run(gpu_ctx, ns, [(ns[0] * ns[0], 1, 1, 1, 0)], 64, True)
    assert e.value.code == _native.FSDKR_E_ARG
    # the fused chain has the 8-lane shape only; the composed path takes any setting
    try:
        for lanes in (4, 16):
            gpu_ctx.set_modexp_group(lanes)
            with pytest.raises(_native.FsdkrError) as e:
                _run(gpu_ctx, ns, inst[:3], 64, True)
            assert e.value.code == _native.FSDKR_E_ARG
            assert _run(gpu_ctx, ns, inst[:3], 64, False) == want[:3]
        gpu_ctx.set_modexp_group(8)
        assert _run(gpu_ctx, ns, inst[:9], 64, True) == want[:9]
    finally:
        gpu_ctx.set_modexp_group(0)


# ---- 4 / 5. mta.respond end to end: the reference's bob_zkp on the device ---------
class _Replay:
    """sample_below from a queue of preset draws (each checked against its bound),
    then from a real Rng: respond's beta' / r are the scenario's, its proofs' draws
    are a seeded stream."""

    def __init__(self, preset, then):
        self.preset, self.then = list(preset), then

    def sample_below(self, upper):
        if self.preset:
            bound, v = self.preset.pop(0)
            assert upper == bound and v < upper
            return v
        return self.then.sample_below(upper)


@pytest.fixture(scope="module")
def exchanges(gpu_ctx, keys):
    """6 exchanges over the two key sets: Alice's a and Enc(a) made on the device,
    the oracle's scenario values, and respond's outputs (plain and with check)."""
    from fsdkr import mta
    sets = keys["sets"]
    ex = []
    for k in range(6):
        key = sets[k % 2]
        seed = ("mta-respond-e2e", k)
        a_enc_o, mta_o, b, beta_prim, r = mo.mta_scenario(key["ek"], Rng(seed))
        rr = Rng(seed)
        a = rr.sample_below(Q)
        r_a = rr.sample_below(key["ek"].n)
        ex.append(dict(key=key, a=a, r_a=r_a, a_enc_o=a_enc_o, mta_o=mta_o, b=b, beta_prim=beta_prim, r=r))
    ns = [s["ek"].n for s in sets]
    a_encs = gpu_ctx.paillier_encrypt([e["a"] for e in ex], [e["r_a"] for e in ex], ns, [k % 2 for k in range(6)], 64)
    assert a_encs == [e["a_enc_o"] for e in ex]
    eks, sts = [e["key"]["ek"] for e in ex], [e["key"]["st"] for e in ex]
    res = {}
    for check in (False, True):
        preset = [(e["key"]["ek"].n, v) for e in ex for v in (e["beta_prim"], e["r"])]
        rng = _Replay(preset, Rng(("mta-respond-proofs", check)))
        res[check] = mta.respond(a_encs, [e["b"] for e in ex], eks, sts, rng, ctx=gpu_ctx, check=check)
        assert not rng.preset
    return ex, a_encs, eks, sts, res


def test_respond_end_to_end(gpu_ctx, exchanges):
    from fsdkr import mta
    ex, a_encs, eks, sts, res = exchanges
    for check in (False, True):
        mta_outs, betas, proofs = res[check]
        assert mta_outs == [e["mta_o"] for e in ex]
        assert betas == [(-e["beta_prim"]) % Q for e in ex]
        X = [ec.mul(ec.G, e["b"]) for e in ex] if check else None
        assert list(mta.verify_bob(proofs, a_encs, mta_outs, eks, sts, X=X, ctx=gpu_ctx)) == [1] * 6
        assert [mo.outcome(p, a, m, ek, st, x) for p, a, m, ek, st, x in
                zip(proofs, a_encs, mta_outs, eks, sts, X or [None] * 6)] == [1] * 6
    mta_outs, betas, _ = res[False]
    alphas = mta.finish(mta_outs, [e["key"]["dk"] for e in ex], ctx=gpu_ctx)
    assert [paillier.decrypt(e["key"]["dk"], m) % Q for e, m in zip(ex, mta_outs)] == alphas
    assert [(al + be) % Q for al, be in zip(alphas, betas)] == [e["a"] * e["b"] % Q for e in ex]
    one = mta.finish(mta_outs[:1], [ex[0]["key"]["dk"]], ctx=gpu_ctx)   # a single key: paillier_decrypt
    assert one == alphas[:1]


def test_respond_proofs_are_generate_bobs(gpu_ctx, exchanges):
    """The same Rng seed: respond's proofs are generate_bob's on the oracle-made mta_out."""
    from fsdkr import mta
    ex, a_encs, eks, sts, res = exchanges
    for check in (False, True):
        items = [(a, e["mta_o"], e["b"], e["beta_prim"], e["key"]["ek"], e["key"]["st"], e["r"])
                 for a, e in zip(a_encs, ex)]
        want = mta.generate_bob(items, Rng(("mta-respond-proofs", check)), ctx=gpu_ctx, check=check)
        assert res[check][2] == want
