"""Proofs whose Fiat-Shamir transcripts have chosen byte lengths, for the device
hashes of fs-dkr_amd/csrc/vhash.hip (alice_hash / alice_prefix / bob_hash /
ped_hash over the streaming SHA-256 of csrc/sha256.hpp).

Honest proofs under full-width keys have fixed transcript lengths (a multiple of
64 bytes), so the paths selected by a length -- the three misaligned word()
appends with their block rollover, finish_le() at 55 | 56..63 | 0 pending bytes,
a saved prefix state that ends inside a word, N + 1 growing a limb, and
ped_hash's per-value lengths and chunking -- are reached by chance at most.  The
verifiers check nothing about how the prover drew its randomness and hash the
values as given, so the lengths can be chosen exactly:

  Alice   statement h1 = 2, prover's ro = 0: z = 2^a, a // 8 + 1 bytes
  Bob     the same with z = 2^b, and sigma = 0: t = 2^beta'
  ring-Pedersen   T = 2, S = 2^lambda, A_i = 2^a_i, Z_i = a_i + e_i lambda
                  (and the same over T = 3, whose powers have no zero bytes to
                  hide a byte that ped_hash's scatter put in the wrong place)

N and N~ are random odd numbers of an exact bit length (verification needs no
factorisation); r, beta and h2 are drawn as units, and everything but the scripted
draws stays random, so the arithmetic kernels see ordinary operands.

This file (CPU only) holds the builders and proves, with the oracle and hashlib
alone, what tests/test_hash_lengths_gpu.py relies on: (a) the oracle accepts
every case, (b) every target residue of the transcript length mod 64 is present
and the later values start at every byte offset mod 4, (c) tampers that change
nothing but the digest exist and the oracle rejects them."""
import copy
import dataclasses
import functools
import hashlib

import pytest

import mta_oracle as mo
from oracle import bigint, protocol
from oracle import range_proofs as rp
from oracle import ring_pedersen
from oracle import secp256k1 as ec
from oracle.hashing import chain_bigint
from oracle.paillier import EncryptionKey
from oracle.ring_pedersen import RingPedersenProof, RingPedersenStatement
from oracle.rng import Rng
from oracle.zk_paillier import DLogStatement

Q = ec.Q
Q3 = Q ** 3
KB = 1024     # the collect() sessions' key size

R64 = tuple(range(64))
# the padding edge 55 | 56, the four word() alignments at the start and at the finish, the block boundary
B = (0, 1, 2, 3, 4, 31, 32, 33, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63)
B6 = (0, 3, 55, 56, 58, 63)


def blen(v):
    """Bytes of BigInt::to_bytes(v)."""
    return len(bigint.to_bytes(v))


class Replay:
    """An rng for the oracle's provers that hands out the given draws in order."""

    def __init__(self, draws):
        self.draws = list(draws)

    def sample_below(self, bound):
        v = self.draws.pop(0)
        assert 0 <= v < bound
        return v

    def from_modulo(self, n):
        v = self.draws.pop(0)
        assert 0 <= v < n and bigint.gcd(v, n) == 1
        return v


def odd_modulus(rng, bits, top_byte=None):
    """A random odd number of exactly `bits` bits (top_byte: its leading byte, bits % 8 == 0)."""
    n = rng.bits(bits) | (1 << (bits - 1)) | 1
    if top_byte is not None:
        n = (n & ((1 << (bits - 8)) - 1)) | (top_byte << (bits - 8))
    return n


def verifier_key(nbits, tbits, seed, ones=False):
    """(ek, statement): N of nbits bits (ones: 2^nbits - 1, so N + 1 grows a limb),
    N~ of tbits bits, h1 = 2 and a random unit h2."""
    rng = Rng(("hash-len-key", nbits, tbits, seed))
    n = (1 << nbits) - 1 if ones else odd_modulus(rng, nbits)
    nt = odd_modulus(rng, tbits)
    return EncryptionKey.from_n(n), DLogStatement(nt, 2, rng.from_modulo(nt))


def _class_limbs(ek, st):
    return 64 if max(ek.n.bit_length(), st.N.bit_length()) <= 2048 else 96


# ------------------------------------------------------------------ Alice ------
def _alice_case(ek, st, target, seed, k):
    rng = Rng(("hash-len-alice", seed, k))
    n, nn, nt = ek.n, ek.nn, st.N
    r = rng.from_modulo(n)
    alpha, beta, gamma = rng.sample_below(Q3), rng.from_modulo(n), rng.sample_below(Q3 * nt)
    # u and w do not depend on a: their lengths are known before a is chosen
    u = (alpha * n + 1) * bigint.mod_pow(beta, n, nn) % nn
    w = bigint.mod_pow(st.g, alpha, nt) * bigint.mod_pow(st.ni, gamma, nt) % nt
    rn = bigint.mod_pow(r, n, nn)
    fixed = blen(n) + blen(n + 1) + blen(u) + blen(w)
    lc = blen(nn)
    for it in range(8):
        lz = (target - fixed - lc) % 64 or 64
        a = 8 * (lz - 1) + (k + it) % 8
        c = (a * n + 1) * rn % nn
        if blen(c) == lc:
            break
        lc = blen(c)
    else:
        raise AssertionError("no a for the target length")
    pf = rp.generate(a, c, ek, st, r, Replay([alpha, beta, gamma, 0]))
    assert pf.z == 1 << a and pf.e == chain_bigint(n, n + 1, c, pf.z, u, w)
    return dict(pf=pf, cipher=c, ek=ek, st=st, target=target,
                lens=tuple(blen(v) for v in (n, n + 1, c, pf.z, u, w)))


def alice_cases(nbits, tbits, targets, seed, ones=False):
    """One AliceProof per target: its transcript N, N+1, c, z, u, w has target mod 64
    bytes.  Each case: pf, cipher, ek, st, target and lens, the byte length of the
    six hashed values."""
    ek, st = verifier_key(nbits, tbits, seed, ones)
    return list(bigint.pool().map(lambda kt: _alice_case(ek, st, kt[1], seed, kt[0]), enumerate(targets)))


def alice_tampers(cases):
    """(kind, case) rows that differ from an accepted case in the digest alone: e ^ 1,
    and z + N~ / cipher + N^2 (equal residues of another length, hashed as given)
    where the call's width class has room."""
    rows = []
    for c in (cases[0], cases[-1]):
        rows.append(("e^1", dict(c, pf=dataclasses.replace(c["pf"], e=c["pf"].e ^ 1))))
    nl = _class_limbs(cases[0]["ek"], cases[0]["st"])
    c = cases[len(cases) // 2]
    if (c["pf"].z + c["st"].N).bit_length() <= 32 * nl:
        rows.append(("z+Nt", dict(c, pf=dataclasses.replace(c["pf"], z=c["pf"].z + c["st"].N))))
    if (c["cipher"] + c["ek"].nn).bit_length() <= 64 * nl:
        rows.append(("c+NN", dict(c, cipher=c["cipher"] + c["ek"].nn)))
    return rows


def alice_verdicts(cases):
    return list(bigint.pool().map(lambda c: int(rp.verify(c["pf"], c["cipher"], c["ek"], c["st"])), cases))


ALICE_SETS = {
    "r64": dict(nbits=2048, tbits=2048, targets=R64, seed="r64"),
    "narrow": dict(nbits=2041, tbits=2033, targets=B, seed="narrow"),
    "ones64": dict(nbits=2048, tbits=2048, targets=(0, 55, 56, 63), seed="ones64", ones=True),
    "b96": dict(nbits=3072, tbits=3072, targets=B, seed="b96"),
    "ones96": dict(nbits=3072, tbits=3072, targets=(55, 56), seed="ones96", ones=True),
}


@functools.lru_cache(maxsize=None)
def alice_set(name):
    """(cases, tampers, oracle verdicts of cases + tampers) of ALICE_SETS[name]."""
    cases = alice_cases(**ALICE_SETS[name])
    tampers = alice_tampers(cases)
    return cases, tampers, alice_verdicts(cases + [t[1] for t in tampers])


def alice_offsets(case):
    """Byte offsets at which u and w start."""
    ln = case["lens"]
    return sum(ln[:4]), sum(ln[:5])


# -------------------------------------------------------------------- Bob ------
def _bob_case(ek, st, target, seed, k, ext):
    rng = Rng(("hash-len-bob", seed, k, ext))
    n, nn, nt = ek.n, ek.nn, st.N
    a_enc = (rng.sample_below(Q) * n + 1) * bigint.mod_pow(rng.from_modulo(n), n, nn) % nn
    r = rng.from_modulo(n)
    alpha, beta, gamma = rng.sample_below(Q3), rng.from_modulo(n), rng.sample_below(Q * Q * n)
    ro_prim, tau = rng.sample_below(Q3 * nt), rng.sample_below(Q3 * nt)
    # z', v, w do not depend on b or beta'
    z_prim = bigint.mod_pow(st.g, alpha, nt) * bigint.mod_pow(st.ni, ro_prim, nt) % nt
    w = bigint.mod_pow(st.g, gamma, nt) * bigint.mod_pow(st.ni, tau, nt) % nt
    v = bigint.mod_pow(a_enc, alpha, nn) * (gamma * n + 1) * bigint.mod_pow(beta, n, nn) % nn
    rn = bigint.mod_pow(r, n, nn)
    beta_prim = 8 * ((k // 3) % 4) + k % 8            # t = 2^beta': 1 to 4 bytes, out of step with the targets
    t = 1 << beta_prim
    u_pt = ec.mul(ec.G, alpha) if ext else None
    fixed = sum(blen(x) for x in (n, n + 1, a_enc, z_prim, t, v, w)) + (blen(u_pt[0]) + blen(u_pt[1]) if ext else 0)
    var = blen(nn) + (64 if ext else 0)                # mta and X's coordinates: they depend on b
    for it in range(8):
        lz = (target - fixed - var) % 64 or 64
        b = 8 * (lz - 1) + 1 + (k + it) % 7            # b >= 1: X = b G is a point
        mta = bigint.mod_pow(a_enc, b, nn) * (beta_prim * n + 1) % nn * rn % nn
        X = ec.mul(ec.G, b) if ext else None
        got = blen(mta) + (blen(X[0]) + blen(X[1]) if ext else 0)
        if got == var:
            break
        var = got
    else:
        raise AssertionError("no b for the target length")
    draws = Replay([alpha, beta, gamma, 0, ro_prim, 0, tau])
    pf, u = mo.generate(a_enc, mta, b, beta_prim, ek, st, r, draws, check=ext)
    assert pf.z == 1 << b and pf.t == t and u == u_pt
    vals = [n, n + 1, a_enc, mta, pf.z, z_prim, pf.t, v, w] + ([X[0], X[1], u[0], u[1]] if ext else [])
    assert pf.e == chain_bigint(*vals)
    return dict(pf=mo.BobProofExt(pf, u) if ext else pf, a_enc=a_enc, mta=mta, X=X, ek=ek, st=st, target=target,
                lens=tuple(blen(x) for x in vals))


def bob_cases(nbits, tbits, targets, seed, ext, ones=False):
    """One BobProof (ext: BobProofExt with X = b G) per target, as alice_cases; the
    transcript is N, N+1, a_enc, mta, z, z', t, v, w [, X.x, X.y, u.x, u.y]."""
    ek, st = verifier_key(nbits, tbits, seed, ones)
    return list(bigint.pool().map(lambda kt: _bob_case(ek, st, kt[1], seed, kt[0], ext), enumerate(targets)))


def bob_tampers(cases):
    rows = []
    for c in (cases[0], cases[-1]):
        inner = c["pf"].proof if hasattr(c["pf"], "proof") else c["pf"]
        rows.append(("e^1", dict(c, pf=mo.with_field(c["pf"], "e", inner.e ^ 1))))
    nl = _class_limbs(cases[0]["ek"], cases[0]["st"])
    c = cases[len(cases) // 2]
    inner = c["pf"].proof if hasattr(c["pf"], "proof") else c["pf"]
    if (inner.z + c["st"].N).bit_length() <= 32 * nl:
        rows.append(("z+Nt", dict(c, pf=mo.with_field(c["pf"], "z", inner.z + c["st"].N))))
    if (inner.t + c["st"].N).bit_length() <= 32 * nl:
        rows.append(("t+Nt", dict(c, pf=mo.with_field(c["pf"], "t", inner.t + c["st"].N))))
    if (c["mta"] + c["ek"].nn).bit_length() <= 64 * nl:
        rows.append(("mta+NN", dict(c, mta=c["mta"] + c["ek"].nn)))
    return rows


def bob_verdicts(cases):
    return list(bigint.pool().map(lambda c: mo.outcome(c["pf"], c["a_enc"], c["mta"], c["ek"], c["st"], c["X"]), cases))


BOB_SETS = {
    "plain64": dict(nbits=2048, tbits=2048, targets=B, seed="plain64", ext=False),
    "ext64": dict(nbits=2041, tbits=2033, targets=B, seed="ext64", ext=True),
    "plain96": dict(nbits=3072, tbits=3072, targets=B6, seed="plain96", ext=False),
    "ones64": dict(nbits=2048, tbits=2048, targets=(55,), seed="ones64", ext=False, ones=True),
    "ones96": dict(nbits=3072, tbits=3072, targets=(56,), seed="ones96", ext=True, ones=True),
}


@functools.lru_cache(maxsize=None)
def bob_set(name):
    cases = bob_cases(**BOB_SETS[name])
    tampers = bob_tampers(cases)
    return cases, tampers, bob_verdicts(cases + [t[1] for t in tampers])


def bob_offsets(case):
    """Byte offsets at which z', v and w start."""
    ln = case["lens"]
    return sum(ln[:5]), sum(ln[:7]), sum(ln[:8])


# ---------------------------------------------------------- ring-Pedersen ------
def rp_outcome(pf, st, M):
    """1 accepted, 0 rejected, 2 the reference panics (a digest shorter than M bits)."""
    try:
        return int(ring_pedersen.verify(pf, st, M))
    except bigint.PanicError:
        return 2


def rp_case(nl_bits, a_list, seed, T=2):
    """A ring-Pedersen proof over T = 2 with A_i = 2^a_i mod N (as given for 2^a_i < N)
    for an odd N of nl_bits bits, and its digest-only tamper A_0 T, Z_0 + 1.  A
    digest shorter than M bits is kept (Z for the readable bits): the oracle's
    outcome is then its panic.  T = 3 gives values of chosen lengths whose bytes
    are all in use (2^a is one byte over zeros, which hides a misplaced byte inside
    a value).  Returns st, pf, bad, M, lens (bytes of every A_i)."""
    rng = Rng(("hash-len-rp", nl_bits, seed))
    M = len(a_list)
    n = odd_modulus(rng, nl_bits)
    lam = rng.sample_below(n)
    st = RingPedersenStatement(bigint.mod_pow(T, lam, n), T, n, 0, EncryptionKey.from_n(n))
    A = [bigint.mod_pow(T, a, n) for a in a_list]
    eb = bigint.to_bytes(chain_bigint(*A))
    Z = [a + (((eb[i >> 3] >> (i & 7)) & 1) * lam if i < 8 * len(eb) else 0) for i, a in enumerate(a_list)]
    pf = RingPedersenProof(tuple(A), tuple(Z))
    bad = RingPedersenProof((A[0] * T % n,) + tuple(A[1:]), (Z[0] + 1,) + tuple(Z[1:]))
    return dict(st=st, pf=pf, bad=bad, M=M, lens=tuple(blen(a) for a in A))


def _exp_for(nbytes, j):
    """An exponent a with 2^a of nbytes bytes."""
    return 8 * (nbytes - 1) + j % 8


def _exp3_for(nbytes, j):
    """An exponent a with 3^a of nbytes bytes and below 2^(8 nbytes - 2)."""
    a = int(8 * (nbytes - 1) / 1.585)
    while blen(3 ** a) < nbytes:
        a += 1
    a += j % 3 if nbytes > 1 else 0
    assert blen(3 ** a) == nbytes and (3 ** a).bit_length() <= max(2, 8 * nbytes - 2)
    return a


def rp_mixed(M, nl, seed, T=2):
    """Exponents for value lengths 1, 2, 3, 4, 5, 4k, 4k + 1 and the full 4 nl bytes, then seeded lengths."""
    rng = Rng(("hash-len-rp-mixed", M, nl, seed))
    full = 4 * nl
    head = [1, 2, 3, 4, 5, 8, 9, full, 12, 13, full - 1, 6, 7, 16, full - 3, 17, full]
    lens = [head[i] if i < len(head) else 1 + rng.sample_below(full) for i in range(M)]
    return [(_exp_for if T == 2 else _exp3_for)(L, rng.sample_below(8)) for L in lens]


def _rp_sets():
    sets = {}
    for M in (16, 17, 31, 32, 33, 48, 255, 256):
        sets[f"mixed{M}"] = (2048, rp_mixed(M, 64, "m"), f"mixed{M}")
    for M in (55, 56, 64, 17, 33):          # every A_i = 1: M bytes in all
        sets[f"ones{M}"] = (2048, [0] * M, f"ones{M}")
    # nl = 96: a first chunk of 63 bytes, then sixteen 384-byte values behind it
    sets["occupancy96"] = (3072, [_exp_for(4, i) for i in range(15)] + [_exp_for(3, 5)] + [3071] * 16, "occ")
    # T = 3: the same length profiles with every byte in use; carry63: a chunk of 64 + 63 bytes,
    # so 63 bytes move to the front behind a compressed block
    for M in (33, 48, 256):
        sets[f"dense{M}"] = (2048, rp_mixed(M, 64, "d", 3), f"dense{M}", 3)
    sets["dense_occupancy96"] = (3072, [_exp3_for(4, i) for i in range(15)] + [_exp3_for(3, 1)] +
                                 [_exp3_for(384, i) for i in range(16)], "dense-occ", 3)
    sets["dense_carry63"] = (2048, [_exp3_for(8, i) for i in range(15)] + [_exp3_for(7, 2)] + rp_mixed(17, 64, "c", 3),
                             "dense-carry", 3)
    return sets


RP_SETS = _rp_sets()
# one call, M = 33, five length profiles
RP_MULTI = ((2048, [0] * 33, "multi-ones"), (2048, [2047] * 33, "multi-full"), (2048, rp_mixed(33, 64, "x"), "multi-x"),
            (2041, [_exp_for(2, i) for i in range(33)], "multi-two"), (2048, rp_mixed(33, 64, "y"), "multi-y"),
            (1999, [_exp_for(1 + 7 * i, i) for i in range(33)], "multi-ramp"),
            (2048, rp_mixed(33, 64, "z", 3), "multi-dense", 3),
            (2040, [_exp3_for(255 - 7 * i, i) for i in range(33)], "multi-dense-ramp", 3))


def _rp_built(spec):
    c = rp_case(*spec)
    want = [rp_outcome(p, c["st"], c["M"]) for p in (c["pf"], c["bad"])]   # verify maps over the pool itself
    return c, want


@functools.lru_cache(maxsize=None)
def rp_set(name):
    """(case, [oracle outcome of pf, of bad]) of RP_SETS[name]."""
    return _rp_built(RP_SETS[name])


@functools.lru_cache(maxsize=None)
def rp_multi():
    return [_rp_built(spec) for spec in RP_MULTI]


# ------------------------------------------------- collect(): prefix handoff ---
# bytes of the receivers' N~ in the two sessions: with 1024-bit Paillier keys N, N + 1 and c
# fill 512 bytes, so the prefix N, N+1, c, z ends len(z) = len(N~) bytes past a block boundary
COLLECT_NT_BYTES = ((128, 65, 66, 67, 119), (120, 127, 64, 121, 96))
COLLECT_TARGETS = (0, 1, 2, 3, 55, 56, 63)
COLLECT_PARTY = (0, 1)                       # the collecting party's position, per session
COLLECT_TAMPER = ((2, 1), (3, 1))            # (message, receiver) whose range proof gets e ^ 1


@functools.lru_cache(maxsize=None)
def collect_sessions():
    """Two t = 2, n = 5 refresh sessions whose receivers' (N~, h1, h2) are statements
    over odd N~ of COLLECT_NT_BYTES bytes, replaced BEFORE distribute so that the
    oracle's own prover makes every PDL and range proof over them.  Per session:
    keys, msgs, dks and prefix[k][i], the bytes of N_i, N_i + 1, c, z of message k's
    range proof for receiver i."""
    rng = Rng("hash-len-collect")
    base = protocol.simulate_keygen(2, 5, rng, KB)
    out = []
    for s, nt_bytes in enumerate(COLLECT_NT_BYTES):
        keys = [k.clone() for k in base]
        sts = []
        for L in nt_bytes:   # a leading 0xff byte: z < N~ has N~'s length but for one draw in 256
            nt = odd_modulus(rng, 8 * L, top_byte=0xFF)
            sts.append(DLogStatement(nt, rng.from_modulo(nt), rng.from_modulo(nt)))
        msgs, dks = [], []
        for key in keys:
            key.h1_h2_n_tilde_vec = list(sts)
            m, dk = protocol.distribute(key.i, key, 5, rng, KB)
            msgs.append(m)
            dks.append(dk)
        prefix = [[sum(blen(v) for v in (keys[0].paillier_key_vec[i].n, keys[0].paillier_key_vec[i].n + 1,
                                         m.points_encrypted_vec[i], m.range_proofs[i].z)) for i in range(5)]
                  for m in msgs]
        out.append(dict(keys=keys, msgs=msgs, dks=dks, prefix=prefix))
    return out


def collect_tampered(s):
    """Session s with one pair's range proof carrying e ^ 1."""
    k, i = COLLECT_TAMPER[s]
    msgs = copy.deepcopy(collect_sessions()[s]["msgs"])
    a = msgs[k].range_proofs[i]
    msgs[k].range_proofs[i] = dataclasses.replace(a, e=a.e ^ 1)
    return msgs


@functools.lru_cache(maxsize=None)
def collect_oracle(s, tampered):
    """(outcome, LocalKey after) of the oracle's collect on session s."""
    ses = collect_sessions()[s]
    key = ses["keys"][COLLECT_PARTY[s]].clone()
    msgs = collect_tampered(s) if tampered else copy.deepcopy(ses["msgs"])
    try:
        protocol.collect(msgs, key, ses["dks"][COLLECT_PARTY[s]], [], Rng("a8"), KB)
    except protocol.FsDkrError as e:
        return (e.variant, e.fields), key
    return None, key


# ---------------------------------------------------------------- the tests ----
@pytest.mark.parametrize("name", sorted(ALICE_SETS))
def test_alice_cases(name):
    cases, tampers, want = alice_set(name)
    targets = ALICE_SETS[name]["targets"]
    # (a) accepted, (c) the tampers rejected
    assert want == [1] * len(cases) + [0] * len(tampers)
    # (b) every target residue, none missing
    assert sorted(sum(c["lens"]) % 64 for c in cases) == sorted(targets)
    for c in cases:
        vals = (c["ek"].n, c["ek"].n + 1, c["cipher"], c["pf"].z)
        assert c["lens"][:4] == tuple(blen(v) for v in vals)
        z = c["pf"].z
        assert c["st"].g == 2 and z & (z - 1) == 0 and c["lens"][3] == (z.bit_length() - 1) // 8 + 1
    kinds = [t[0] for t in tampers]
    assert kinds.count("e^1") == 2
    if name == "narrow":
        assert "z+Nt" in kinds and "c+NN" in kinds
        assert all(c["lens"][0] == 256 and c["lens"][1] == 256 for c in cases)   # 2041 bits: one zero byte on top
    if ALICE_SETS[name].get("ones"):
        nb = ALICE_SETS[name]["nbits"] // 8
        assert all(c["lens"][:2] == (nb, nb + 1) for c in cases)                 # N + 1 grew a limb
    if len(targets) >= len(B):
        for which in (0, 1):
            assert {alice_offsets(c)[which] % 4 for c in cases} == {0, 1, 2, 3}


def test_alice_tampers_change_only_the_digest():
    cases, tampers, _ = alice_set("narrow")
    src = cases[len(cases) // 2]
    for kind, t in tampers:
        if kind == "z+Nt":   # the same residue, 255 bytes where z had at most 64
            assert t["pf"].z % t["st"].N == src["pf"].z and t["cipher"] == src["cipher"]
            assert blen(t["pf"].z) == 255 > blen(src["pf"].z) and t["pf"].z.bit_length() <= 2048
        if kind == "c+NN":
            assert t["cipher"] % t["ek"].nn == src["cipher"] and t["pf"] == src["pf"]
            assert t["cipher"] != src["cipher"] and t["cipher"].bit_length() <= 4096


@pytest.mark.parametrize("name", sorted(BOB_SETS))
def test_bob_cases(name):
    cases, tampers, want = bob_set(name)
    spec = BOB_SETS[name]
    assert want == [1] * len(cases) + [0] * len(tampers)
    assert sorted(sum(c["lens"]) % 64 for c in cases) == sorted(spec["targets"])
    assert all(len(c["lens"]) == (13 if spec["ext"] else 9) for c in cases)
    kinds = [t[0] for t in tampers]
    assert kinds.count("e^1") == 2
    if name == "ext64":
        assert {"z+Nt", "t+Nt", "mta+NN"} <= set(kinds)
    if spec.get("ones"):
        nb = spec["nbits"] // 8
        assert all(c["lens"][:2] == (nb, nb + 1) for c in cases)
    if len(spec["targets"]) >= len(B):
        for which in (0, 1, 2):
            assert {bob_offsets(c)[which] % 4 for c in cases} == {0, 1, 2, 3}
        assert {c["lens"][6] for c in cases} == {1, 2, 3, 4}                      # t = 2^beta'


@pytest.mark.parametrize("name", sorted(RP_SETS))
def test_rp_cases(name):
    c, want = rp_set(name)
    M = c["M"]
    digest = hashlib.sha256(b"".join(bigint.to_bytes(a) for a in c["pf"].A)).digest()
    short = 8 * blen(int.from_bytes(digest, "big")) < M   # the oracle panics at the first unreadable bit
    assert want == [2 if short else 1, 0]
    assert c["bad"].A[1:] == c["pf"].A[1:] and c["bad"].Z[1:] == c["pf"].Z[1:]
    assert c["bad"].A[0] == c["pf"].A[0] * c["st"].T % c["st"].N and c["bad"].Z[0] == c["pf"].Z[0] + 1
    lens = c["lens"]
    if name.startswith("ones"):
        assert lens == (1,) * M and sum(lens) == M
    if name.startswith("mixed") or name in ("dense33", "dense48", "dense256"):
        assert {1, 2, 3, 4, 5, 8, 9, 12, 13, 256} <= set(lens) and sum(lens) % 64 != 0
        assert c["st"].N > 1 << 2047
    if name.endswith("occupancy96"):
        assert sum(lens[:16]) == 63 and lens[16:] == (384,) * 16
    if name == "dense_carry63":
        assert sum(lens[:16]) == 64 + 63
    if name.startswith("dense"):   # as given (below N), and no run of zero bytes to hide a misplaced one
        assert c["st"].T == 3 and all(a == 3 ** x for a, x in zip(c["pf"].A, RP_SETS[name][1]))


def test_rp_multi_profiles():
    built = rp_multi()
    assert len(built) >= 5 and len({c["M"] for c, _ in built}) == 1
    assert len({c["lens"] for c, _ in built}) == len(built)
    assert len({sum(c["lens"]) % 64 for c, _ in built}) >= 4
    assert [w for _, w in built] == [[1, 0]] * len(built)


def test_collect_sessions_cover_the_prefix_residues():
    sessions = collect_sessions()
    got = {p % 64 for ses in sessions for row in ses["prefix"] for p in row}
    assert set(COLLECT_TARGETS) <= got, sorted(got)
    # the residue of the tampered pair is one of the targets
    for s, (k, i) in enumerate(COLLECT_TAMPER):
        assert sessions[s]["prefix"][k][i] % 64 in COLLECT_TARGETS
    for s, ses in enumerate(sessions):
        assert [blen(st.N) for st in ses["keys"][0].h1_h2_n_tilde_vec] == list(COLLECT_NT_BYTES[s])


@pytest.mark.parametrize("s", [0, 1])
def test_collect_sessions_oracle_outcomes(s):
    out, _ = collect_oracle(s, False)
    assert out is None
    out, _ = collect_oracle(s, True)
    assert out == ("RangeProof", {"party_index": COLLECT_TAMPER[s][1]})


@pytest.mark.parametrize("s", [0, 1])
def test_collect_host_packing_takes_narrow_n_tilde(s):
    from fsdkr.batch import CollectBatch
    ses = collect_sessions()[s]
    b = CollectBatch(ses["msgs"], ses["keys"][COLLECT_PARTY[s]], [], 256, KB)
    assert b.n == 5
