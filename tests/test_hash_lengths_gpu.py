"""The device Fiat-Shamir hashes at every transcript-length edge: the verifiers'
verdicts on the proofs of tests/test_hash_lengths.py (chosen byte lengths; the
CPU file proves the coverage and the oracle's outcomes) against the oracle's.

An accept is the strong assertion: alice_hash / bob_hash accept only if the
device's digest equals e in all 256 bits, ring-Pedersen only if all M challenge
bits agree.  Every call also carries tampers that change nothing but the digest
(expected 0).  Expectations come from oracle.range_proofs.verify,
mta_oracle.outcome, oracle.ring_pedersen.verify and oracle.protocol.collect."""
import copy

import pytest

import test_hash_lengths as hl

pytestmark = pytest.mark.gpu


# ------------------------------------------------------- alice_hash_kernel ------
def _verify_alice(ctx, rows):
    from fsdkr import mta
    return list(mta.verify_alice([c["pf"] for c in rows], [c["cipher"] for c in rows], [c["ek"] for c in rows],
                                 [c["st"] for c in rows], ctx=ctx))


@pytest.mark.parametrize("name", ["r64", "narrow", "ones64", "b96", "ones96"])
def test_alice_hash_lengths(gpu_ctx, name):
    """One verify_alice call per set: every residue of the set accepted, the tampers
    rejected.  r64: all 64 residues under a (2048, 2048)-bit key; narrow: a
    (2041, 2033)-bit key, zero-extended; ones64 / ones96: N = 2^2048 - 1 / 2^3072 - 1,
    where N + 1 takes the extra limb; b96: the 96-limb class."""
    cases, tampers, want = hl.alice_set(name)
    assert want[:len(cases)] == [1] * len(cases)
    assert _verify_alice(gpu_ctx, cases + [t[1] for t in tampers]) == want


def test_alice_hash_2048_row_in_the_3072_class(gpu_ctx):
    """The 2048-bit rows of r64 at the residues of B, in one call with a 3072-bit
    row: the call runs in the 96-limb class, the narrower key zero-extended."""
    cases, tampers, want = hl.alice_set("r64")
    idx = [k for k, c in enumerate(cases) if c["target"] in hl.B] + [len(cases) + k for k in range(len(tampers))]
    assert len(idx) == len(hl.B) + len(tampers)
    rows = cases + [t[1] for t in tampers]
    wide, _, wide_want = hl.alice_set("b96")
    got = _verify_alice(gpu_ctx, [rows[k] for k in idx] + wide[:1])
    assert got == [want[k] for k in idx] + wide_want[:1]


# --------------------------------------------------------- bob_hash_kernel ------
def _verify_bob(ctx, rows, fused):
    from fsdkr import mta
    ext = hasattr(rows[0]["pf"], "proof")
    return list(mta.verify_bob([c["pf"] for c in rows], [c["a_enc"] for c in rows], [c["mta"] for c in rows],
                               [c["ek"] for c in rows], [c["st"] for c in rows],
                               X=[c["X"] for c in rows] if ext else None, ctx=ctx, fused=fused))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["plain64", "ext64", "plain96", "ones64", "ones96"])
def test_bob_hash_lengths(gpu_ctx, name, fused):
    """One verify_bob call per set and chain (the hashed v comes from the fused or the
    three separate chains): 9 values (plain) or 13 (ext, X = b G), both width
    classes, the all-ones N once per class."""
    cases, tampers, want = hl.bob_set(name)
    assert want[:len(cases)] == [1] * len(cases)
    assert _verify_bob(gpu_ctx, cases + [t[1] for t in tampers], fused) == want


# --------------------------------------------------------- ped_hash_kernel ------
def _rp_verdicts(ctx, built, nl):
    """The device's outcomes (1 ok, 0 rejected, 2 the reference panics) of every
    case's proof and tamper, in one call."""
    sts, pfs = [], []
    for c, _ in built:
        sts += [c["st"], c["st"]]
        pfs += [c["pf"], c["bad"]]
    v = ctx.ring_pedersen_verify(sts, pfs, built[0][0]["M"], nl)
    return [1 if b & 1 else 2 if b & 2 else 0 for b in v.tolist()]


@pytest.mark.parametrize("name", sorted(hl.RP_SETS))
def test_ped_hash_lengths(gpu_ctx, name):
    """mixedM: value lengths 1, 2, 3, 4, 5, 4k, 4k + 1 .. 256 bytes at M around the
    16-value chunk; onesM: M one-byte values (55 | 56 bytes, one block and a bare
    padding block, chunks that compress nothing); occupancy96: 63 bytes carried
    into a chunk of sixteen 384-byte values; dense*: the same profiles over T = 3,
    every byte of every value in use; dense_carry63: 63 bytes moved to the front
    behind a compressed block."""
    built = hl.rp_set(name)
    nl = 96 if hl.RP_SETS[name][0] > 2048 else 64
    assert _rp_verdicts(gpu_ctx, [built], nl) == built[1]


def test_ped_hash_blocks_are_independent(gpu_ctx):
    """Eight proofs of different length profiles (and their tampers) in one call."""
    built = hl.rp_multi()
    assert _rp_verdicts(gpu_ctx, built, 64) == [w for _, want in built for w in want]


# ----------------------------------- alice_prefix_kernel -> alice_hash_kernel ---
def _gpu_collect(ctx, msgs, key, dk):
    from fsdkr import refresh
    try:
        refresh.collect(msgs, key, dk, [], ctx=ctx, key_bits=hl.KB)
    except refresh.FsDkrError as e:
        return (e.variant, e.fields)
    except refresh.FsDkrPanic:
        return ("panic", "")
    return None


@pytest.mark.parametrize("tampered", [False, True])
@pytest.mark.parametrize("s", [0, 1])
def test_collect_prefix_handoff(gpu_ctx, s, tampered):
    """collect() over receivers whose N~ has 64 .. 128 bytes: the saved prefix state
    ends inside a word, on a block boundary, and at 55 | 56 | 63 pending bytes."""
    ses = hl.collect_sessions()[s]
    want, ko = hl.collect_oracle(s, tampered)
    assert want == (("RangeProof", {"party_index": hl.COLLECT_TAMPER[s][1]}) if tampered else None)
    party = hl.COLLECT_PARTY[s]
    kg = ses["keys"][party].clone()
    msgs = hl.collect_tampered(s) if tampered else copy.deepcopy(ses["msgs"])
    assert _gpu_collect(gpu_ctx, msgs, kg, ses["dks"][party]) == want
    assert [k.n for k in ko.paillier_key_vec] == [k.n for k in kg.paillier_key_vec]
    if not tampered:
        assert (ko.x_i, ko.y, ko.pk_vec) == (kg.x_i, kg.y, kg.pk_vec)
