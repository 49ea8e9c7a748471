"""GPU checks of Bob's two fused mod-N^2 chains for the 3072-bit class (nl = 96):
the response a_enc^b (1 + beta' N) r^N (fsdkr_mta_respond: the 8-lane head over N's
bits >= 256, then mta_tail_ct6144_kernel) and the commitment v = a_enc^alpha
(1 + gamma N) beta^N (fsdkr_bob_commit_v: the head over N's bits >= 768, then
bob_v_tail_ct6144_kernel).  Fused and composed run against Python's pow bit for bit,
and so against each other.

The moduli need not be products of two primes for that, so they are built to meet
the tails' edges (lo = 256 / 768): full 3072-bit keys, a 2048-bit and a 2049-bit key
in the wide class, low lo bits all ones or all zero but bit 0 (the window look-ahead
across every limb of the shift register), heads of one bit and of none, and N = 3.
Ten keys interleaved instance by instance: every key's run is padded to its wave.
The operands cycle through the edge values of tests/test_mta_respond_gpu.py and
tests/test_bob_v_gpu.py.

Which path ran is read from the context's kernel-time marks: a fused call leaves
launches under mta_tail_ct / bob_v_tail_ct, a composed one leaves none."""
import pytest

import mta_oracle as mo
import test_bob_v_gpu as tv
import test_mta_respond_gpu as tr
from oracle import paillier
from oracle import secp256k1 as ec
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

Q = ec.Q
NL = 96
COUNTS_R = (1, 7, 8, 9, 17, 70)   # around one wave (8 chains), two waves, many blocks of the head
COUNTS_V = (1, 7, 9, 17)
SHORT = (6, 7, 9)                 # rows of _moduli: the keys of at most lo bits


def _moduli(lo, tag):
    rng = Rng(("mta-tail6144-moduli", tag))

    def top(bits):
        return rng.bits(bits) | (1 << (bits - 1)) | 1

    ones = top(3072) | ((1 << lo) - 1)
    sparse = (top(3072) >> lo << lo) | 1
    ns = [top(3072), top(2048), top(2049), ones, top(3072), sparse, top(lo), top(lo - 1), top(lo + 1), 3]
    assert [n.bit_length() for n in ns] == [3072, 2048, 2049, 3072, 3072, 3072, lo, lo - 1, lo + 1, 2]
    assert all(n & 1 for n in ns)
    assert ones & ((1 << lo) - 1) == (1 << lo) - 1 and sparse & ((1 << lo) - 1) == 1
    assert all(ns[k].bit_length() <= lo for k in SHORT)
    return ns


@pytest.fixture(scope="module")
def ref_r():
    """70 responses over the ten keys (seven per key) and their values by pow; every
    count uses a prefix."""
    ns = _moduli(256, "respond")
    inst = tr._instances(ns, max(COUNTS_R), "tail6144")
    return ns, inst, tr._want(ns, inst)


@pytest.fixture(scope="module")
def ref_v():
    """26 instances of v over the ten keys (alpha's 13 edge values twice, against other
    keys the second time) and their values by pow; every count uses a prefix."""
    ns = _moduli(768, "v")
    inst = tv._instances(ns, 26, "tail6144")
    return ns, inst, tv._want(ns, inst)


CASES = {"respond": ("ref_r", tr._run, "mta_tail_ct"), "v": ("ref_v", tv._run, "bob_v_tail_ct")}


def _case(request, what):
    name, run, mark = CASES[what]
    return request.getfixturevalue(name) + (run, mark)


def _launches(ctx, mark):
    return ctx.kernel_time(mark)[1]


# ---- 1. fused and composed against pow -----------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("count", COUNTS_R)
def test_respond_3072_matches_pow(gpu_ctx, ref_r, count, fused):
    ns, inst, want = ref_r
    assert tr._run(gpu_ctx, ns, inst[:count], NL, fused) == want[:count]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("count", COUNTS_V)
def test_commit_v_3072_matches_pow(gpu_ctx, ref_v, count, fused):
    ns, inst, want = ref_v
    assert tv._run(gpu_ctx, ns, inst[:count], NL, fused) == want[:count]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("what", ["respond", "v"])
def test_short_keys_alone(gpu_ctx, request, what, fused):
    """Only the keys of at most lo bits in the call: the launch's window is chosen for
    them and no head has more than one bit."""
    ns, inst, want, run, _ = _case(request, what)
    pick = [i for i, row in enumerate(inst) if row[4] in SHORT]
    assert len(pick) >= 6
    sub = [ns[k] for k in SHORT]
    rows = [inst[i][:4] + (SHORT.index(inst[i][4]),) for i in pick]
    assert run(gpu_ctx, sub, rows, NL, fused) == [want[i] for i in pick]


# ---- 2. which path ran ------------------------------------------------------------------
@pytest.mark.parametrize("what", ["respond", "v"])
def test_fused_call_runs_the_6144_bit_tail(gpu_ctx, request, what):
    """A fused nl = 96 call launches the constant-time tail; a composed one does not."""
    ns, inst, want, run, mark = _case(request, what)
    gpu_ctx.kernel_time_reset()
    assert run(gpu_ctx, ns, inst[:9], NL, True) == want[:9]
    assert _launches(gpu_ctx, mark) > 0
    gpu_ctx.kernel_time_reset()
    assert run(gpu_ctx, ns, inst[:9], NL, False) == want[:9]
    assert _launches(gpu_ctx, mark) == 0


@pytest.mark.parametrize("what", ["respond", "v"])
def test_forced_lanes(gpu_ctx, request, what):
    """192 limbs have the 8-lane head only: forced to 8 lanes the call is the automatic
    one; forced to 4 or 16 it succeeds with the same values on the composed path."""
    ns, inst, want, run, mark = _case(request, what)
    try:
        gpu_ctx.set_modexp_group(8)
        gpu_ctx.kernel_time_reset()
        assert run(gpu_ctx, ns, inst[:9], NL, True) == want[:9]
        assert _launches(gpu_ctx, mark) > 0
        for lanes in (4, 16):
            gpu_ctx.set_modexp_group(lanes)
            gpu_ctx.kernel_time_reset()
            assert run(gpu_ctx, ns, inst[:9], NL, True) == want[:9]
            assert _launches(gpu_ctx, mark) == 0
            assert run(gpu_ctx, ns, inst[:9], NL, False) == want[:9]
    finally:
        gpu_ctx.set_modexp_group(0)


# ---- 3. end to end over device-generated 3072-bit keys -------------------------------
@pytest.fixture(scope="module")
def exchanges(gpu_ctx):
    """4 exchanges over two key sets of 3072 bits (a Paillier key and an N~ each, made
    on the device): Alice's a and Enc(a), Bob's b."""
    rng = Rng("mta-tail6144-e2e")
    sets = tr._key_sets(gpu_ctx, rng, 3072, 2)
    assert all(s["ek"].n.bit_length() > 2048 and s["st"].N.bit_length() > 2048 for s in sets)
    ex = []
    for k in range(4):
        key = sets[k % 2]
        ex.append(dict(key=key, a=rng.sample_below(Q), r_a=rng.sample_below(key["ek"].n), b=rng.sample_below(Q)))
    a_encs = gpu_ctx.paillier_encrypt([e["a"] for e in ex], [e["r_a"] for e in ex], [s["ek"].n for s in sets],
                                      [k % 2 for k in range(4)], NL)
    assert a_encs == [paillier.encrypt_with_chosen_randomness(e["key"]["ek"], e["a"], e["r_a"]) for e in ex]
    return ex, a_encs


def test_respond_end_to_end_3072(gpu_ctx, exchanges):
    from fsdkr import mta
    ex, a_encs = exchanges
    eks, sts = [e["key"]["ek"] for e in ex], [e["key"]["st"] for e in ex]
    gpu_ctx.kernel_time_reset()
    mta_outs, betas, proofs = mta.respond(a_encs, [e["b"] for e in ex], eks, sts, Rng("mta-tail6144-respond"), ctx=gpu_ctx)
    assert _launches(gpu_ctx, "mta_tail_ct") > 0
    assert list(mta.verify_bob(proofs, a_encs, mta_outs, eks, sts, ctx=gpu_ctx)) == [1] * 4
    assert mo.outcome(proofs[0], a_encs[0], mta_outs[0], eks[0], sts[0]) == 1
    alphas = mta.finish(mta_outs, [e["key"]["dk"] for e in ex], ctx=gpu_ctx)
    assert [(al + be) % Q for al, be in zip(alphas, betas)] == [e["a"] * e["b"] % Q for e in ex]


def test_generate_bob_fused_is_the_default_path_3072(gpu_ctx, exchanges):
    """One seed: generate_bob(fused=True), whose v runs the fused 6144-bit chain, gives
    bit for bit the proofs of the default path."""
    from fsdkr import mta
    ex, a_encs = exchanges
    rng = Rng("mta-tail6144-items")
    items = []
    for a_enc, e in zip(a_encs, ex):
        ek = e["key"]["ek"]
        bp, r = rng.sample_below(ek.n), rng.sample_below(ek.n)
        mta_out = paillier.add(ek, paillier.mul(ek, a_enc, e["b"]), paillier.encrypt_with_chosen_randomness(ek, bp, r))
        items.append((a_enc, mta_out, e["b"], bp, ek, e["key"]["st"], r))
    gpu_ctx.kernel_time_reset()
    fused = mta.generate_bob(items, Rng("mta-tail6144-proofs"), ctx=gpu_ctx, fused=True)
    assert _launches(gpu_ctx, "bob_v_tail_ct") > 0
    assert fused == mta.generate_bob(items, Rng("mta-tail6144-proofs"), ctx=gpu_ctx)
