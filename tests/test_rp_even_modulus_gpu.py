"""Ring-Pedersen proofs over EVEN moduli N = 2^k m (m odd) through the public entry
Context.ring_pedersen_verify (fsdkr_ring_pedersen_verify), against
oracle.ring_pedersen.verify: the proof-level face of tests/test_pow2_check_gpu.py.

The Montgomery kernels check T^Z_i == A_i S^e_i modulo m, pow2_check_kernel modulo 2^k.
A valid proof needs no phi: with S = T^lam, A_i = T^a_i (mod N) and Z_i = a_i + e_i lam
left unreduced the check holds for any N and any T, even T included.  Each statement
gets tampers that differ only modulo 2^k, A_j <- (A_j + m 2^t) mod N with the challenge
and Z recomputed for the new A: the Montgomery half still passes, so only the 2-adic
kernel can reject.  The expected verdict is always the oracle's: with an even T and
challenge bit 1 the factor S == 0 (mod 2^k) masks the change and the reference accepts.

Statements, at nl = 64 and 96: k = 1, 4, 5, 32, 33, 64, 65, 16 nl, 32 nl - 2 (there
m = 3), the pure powers N = 2^33 and N = 2^(32 nl - 1) (m = 1: the 2-adic half alone
decides); T odd everywhere, T = 2 odd with a_i, lam < 2^9 (Z on both sides of k), and
T == 0 (mod 2^k).  a_i and lam have about 200 bits except in one statement per width
whose Z is longer than k = 16 nl.  One call mixes an odd N, an even N, N = 2^k, N = 0
(the reference panics: verdict 2) and an even N again, so messages without 2-adic rows
stand between ones that have them."""
import random

import pytest

from oracle import bigint, ring_pedersen
from oracle.paillier import EncryptionKey
from oracle.ring_pedersen import RingPedersenProof, RingPedersenStatement

pytestmark = pytest.mark.gpu

M = 16


def twos(N):
    return (N & -N).bit_length() - 1


def statement(N, T, lam):
    return RingPedersenStatement(pow(T, lam, N), T, N, 0, EncryptionKey.from_n(N))


def proof(st, lam, a, bump=None, commitments=None):
    """The valid proof for the commitments T^a_i; bump = (j, delta): A_j + delta mod N first,
    challenge and Z for the A that is sent."""
    A = list(commitments) if commitments else [pow(st.T, ai, st.N) for ai in a]
    if bump is not None:
        A[bump[0]] = (A[bump[0]] + bump[1]) % st.N
    bits = ring_pedersen.challenge_bits(A, M)
    return RingPedersenProof(tuple(A), tuple(ai + e * lam for ai, e in zip(a, bits)))


def oracle_verdict(pf, st):
    try:
        return int(ring_pedersen.verify(pf, st, M))
    except (bigint.PanicError, ZeroDivisionError, ValueError):
        return 2


def cases(nl):
    """[(label, statement, proof, t or None)]: each statement's honest proof and its tampers."""
    rnd = random.Random(f"rp-even-{nl}")
    W = 32 * nl
    out = []
    shapes = [(k, "odd") for k in (1, 4, 5, 32, 33, 64, 65, 16 * nl, W - 2)]
    shapes += [(k, "2odd") for k in (5, 33, 64, 65, 300, 16 * nl)]
    shapes += [(k, "zero") for k in (4, 32, 65)]
    shapes += [(33, "pure-odd"), (W - 1, "pure-odd"), (33, "pure-2odd"), (W - 1, "pure-zero"), (16 * nl, "odd-longZ")]
    for k, kind in shapes:
        pure = kind.startswith("pure")
        m = 1 if pure else rnd.getrandbits(W - k) | 1 << (W - k - 1) | 1
        N = m << k
        assert (m == 3) == (k == W - 2 and not pure) and N.bit_length() == (k + 1 if pure else W)
        small = kind.endswith("2odd")
        ebits = 9 if small else k + 40 if kind == "odd-longZ" else 200
        if kind.endswith("zero"):
            T = (rnd.randrange(1, m) << k) if m > 1 else 0
        elif small:
            T = 2 * (rnd.getrandbits(N.bit_length() - 3) | 1)
        else:
            T = rnd.randrange(N) | 1
        assert T < N
        lam = rnd.getrandbits(ebits) | 1 << (ebits - 1)
        a = [rnd.getrandbits(ebits) for _ in range(M)]
        st = statement(N, T, lam)
        label = f"k={k} {kind}"
        honest = proof(st, lam, a)
        out.append((label, st, honest, None))
        ts = sorted({0, k - 1, 32 * ((k - 1) // 32)}) if kind != "odd-longZ" else [k - 1]
        for t in ts:
            j = rnd.randrange(M)
            pf = proof(st, lam, a, (j, m << t), honest.A)
            assert pf.A != honest.A and all(x % m == y % m for x, y in zip(pf.A, honest.A))     # same residues modulo m
            out.append((label, st, pf, t))
        if small:       # Z = e tz < 2^10 on both sides of k = 64, 65, 300; all above k = 5, all below k = 16 nl
            zs = [z for _, s2, p, _ in out if s2 is st for z in p.Z]
            assert (k >= 1024 or any(z >= k for z in zs)) and (k < 64 or any(0 < z < k for z in zs))
    return out


@pytest.mark.parametrize("nl", [64, 96])
def test_even_moduli_against_the_oracle(gpu_ctx, nl):
    cs = cases(nl)
    want = [oracle_verdict(pf, st) for _, st, pf, _ in cs]
    # conditions on the inputs: every honest proof verifies, every odd-T tamper is rejected,
    # both verdicts, and a rejected tamper at t = k - 1
    for (label, st, _, t), w in zip(cs, want):
        if t is None:
            assert w == 1, label
        elif "zero" not in label and "2odd" not in label:
            assert w == 0, (label, t)
    assert set(want) == {0, 1}
    top = [label for (label, st, _, t), w in zip(cs, want) if w == 0 and t is not None and t == twos(st.N) - 1]
    assert top, "no rejected tamper at t = k - 1"
    even_t = [w for (label, _, _, t), w in zip(cs, want) if t is not None and ("zero" in label or "2odd" in label)]
    assert 0 in even_t and 1 in even_t          # the masked tampers and the others
    got = gpu_ctx.ring_pedersen_verify([st for _, st, _, _ in cs], [pf for _, _, pf, _ in cs], M, nl).tolist()
    bad = [(cs[i][0], cs[i][3], want[i], got[i]) for i in range(len(cs)) if want[i] != got[i]]
    print(f"nl={nl}: {len(cs)} proofs, oracle accepts {want.count(1)}, {len(bad)} differ")
    assert not bad, f"(statement, t, oracle, device): {bad}"


def test_mixed_batch(gpu_ctx):
    """An odd N, an even N, N = 2^k, N = 0 and an even N again in one call: the 2-adic rows
    of a message are found through p2_first, past messages that have none."""
    nl = 64
    rnd = random.Random("rp-even-mixed")
    W = 32 * nl

    def make(N, tamper_t=None, m=1):
        T = rnd.randrange(N) | 1
        lam = rnd.getrandbits(200)
        a = [rnd.getrandbits(200) for _ in range(M)]
        st = statement(N, T, lam)
        return st, proof(st, lam, a, None if tamper_t is None else (rnd.randrange(M), m << tamper_t))
    m1, m2 = (rnd.getrandbits(W - k) | 1 << (W - k - 1) | 1 for k in (40, 70))
    odd = rnd.getrandbits(W) | 1 << (W - 1) | 1
    zero_st, zero_pf = make(odd)
    zero_st = RingPedersenStatement(zero_st.S, zero_st.T, 0, 0, EncryptionKey.from_n(0))
    for tampered in ((), (1, 2, 4), (4,), (1,), (2,)):
        batch = [make(odd),
                 make(m1 << 40, 39 if 1 in tampered else None, m1),
                 make(1 << 200, 199 if 2 in tampered else None),
                 (zero_st, zero_pf),
                 make(m2 << 70, 64 if 4 in tampered else None, m2)]
        want = [oracle_verdict(pf, st) for st, pf in batch]
        assert want == [1, int(1 not in tampered), int(2 not in tampered), 2, int(4 not in tampered)]
        got = gpu_ctx.ring_pedersen_verify([s for s, _ in batch], [p for _, p in batch], M, nl).tolist()
        print(f"tampered {tampered}: device {got}, oracle {want}")
        assert got == want
